// Attention of the QKVTRT / QKVTRT2 plugins (multiHeadAttnPlugin.cpp; det2trt/models/functions/multi_head_attn.py:12-16)
// on the matrix cores, for any lengths:
//
//   out[b, i, :] = sum_j softmax_j( <q[b, i, :], k[b, j, :]> / sqrt(E) ) v[b, j, :]     q [B, Lq, E], k / v [B, Lkv, E]
//
// E % 16 == 0, 16 <= E <= 128; fp16 (v_mfma_f32_32x32x16_f16) or fp32 (v_mfma_f32_32x32x2_f32: f32 operands, no
// rounding to half anywhere).  The general form of csrc/attention.hip: same orientation, same online softmax, but the
// keys STREAM through in tiles of 32 instead of the head's whole K / V image being staged in LDS, so there is no key
// limit and queries / keys are separate tensors.
//
// A block = 32 queries of one batch x NW waves that split the block's key tiles (wave w takes tiles w, w + NW, ...).
// Per tile of 32 keys a wave computes
//   S^T[key, query] = K Q^T      A = the K rows, read by each lane straight from global memory; B = the Q fragment,
//                                resident in registers for the whole kernel
//   online softmax down the key axis: in the C layout a lane holds 16 keys of ONE query (its partner lane + 32 the
//     other 16), so the running maximum / sum are lane-local plus one exchange with the partner
//   O^T[d, query] += V^T P^T     B = the probabilities straight out of the lane's own registers (the C layout's key
//                                order (r & 3) + 8 (r >> 2) + 4 (lane >> 5) is the k order of the product); A = V^T
//     fp16: the wave stages its V tile in a wave-private LDS slice (16-byte loads; a lane then picks its 8 keys x 1
//           channel per instruction 2 bytes at a time, as attention.hip does).  LDS completes one wave's
//           instructions in order, so the slice needs no barrier.
//     fp32: k = 2 keys per instruction, one per lane half: a lane's A element is V[key][its channel], a coalesced
//           4-byte load from global memory; no LDS.
// and at the end the waves' (maximum, sum, accumulator) meet in LDS in a fixed order; waves 0-3 rescale, add and store
// four channels per lane each.  fp32 scores, maxima, sums and accumulators; fp16 probabilities for the fp16 product.
//
// Key split across blocks (grid.z): when B * ceil(Lq / 32) blocks cannot fill the chip, each block takes a contiguous
// range of key tiles and writes its unnormalised partial result (fp32) with its (maximum, sum) to the caller's
// workspace; a second kernel merges the splits in ascending order.  No atomics anywhere: bit-reproducible.
#include <algorithm>
#include <climits>

#include "common.h"

namespace bevops {
namespace {

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

constexpr int kQkvCUs = 256;        // MI355X
constexpr int kQkvMinE = 16, kQkvMaxE = 128;

struct QkvArgs {
  const void *q, *k, *v;
  void *out;
  float *part_o;    // [nsplit][B * Lq][E] unnormalised partial outputs, or null (one split: normalise and store)
  float *part_ml;   // [nsplit][B * Lq][2] (maximum in log2 units, sum)
  int batch, q_len, kv_len, tiles_per_split;
  float scale_log2e;
};

// scores of one 32-key tile in log2 units (keys past kv_len are -inf) -> probabilities p, rescale factor of the
// running state; m_run / l_run are updated
__device__ __forceinline__ float qkv_online_softmax(f32x16_t &s, float (&p)[16], float &m_run, float &l_run, int k0,
                                                    int kv_len, int hi, float scale_log2e) {
  if (k0 + 32 > kv_len) {                   // (wave-uniform: only the last tile of the sequence is partial)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      s[r] = key < kv_len ? s[r] * scale_log2e : -INFINITY;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] *= scale_log2e;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[r]);
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // the partner lane holds the query's other 16 keys
  const float m_new = fmaxf(m_run, mx);     // finite: every tile holds at least one key
  const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // (first tile: exp2(-inf) = 0)
  m_run = m_new;
  float psum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    p[r] = __builtin_amdgcn_exp2f(s[r] - m_new);
    psum += p[r];
  }
  l_run = l_run * alpha + psum;
  return alpha;
}

__device__ __forceinline__ void qkv_store4(__half *o, float a, float b, float c, float d) {
  uint2 w;
  w.x = pack_h2(a, b);
  w.y = pack_h2(c, d);
  *reinterpret_cast<uint2 *>(o) = w;
}
__device__ __forceinline__ void qkv_store4(float *o, float a, float b, float c, float d) {
  *reinterpret_cast<float4 *>(o) = make_float4(a, b, c, d);
}

// The waves' partial states meet in LDS (the tile slices are dead by now): [NW][2][64] statistics, then per 32-channel
// output tile [NW][16][64] accumulators; wave g < 4 finishes accumulator registers 4g .. 4g + 3 of every tile (channels
// 32 c + 8 g + 4 hi .. + 3 of its lane's query).  Must be reached by every wave of the block.
template <int E, int NW, typename T>
__device__ __forceinline__ void qkv_block_merge(const QkvArgs &a, char *smem, const f32x16_t (&acc)[(E + 31) / 32],
                                                float m_run, float l_run, int b, int q0) {
  constexpr int EC = (E + 31) / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5;
  float *st = reinterpret_cast<float *>(smem);
  float *xa = st + NW * 2 * 64;
  __syncthreads();
  st[wave * 128 + lane] = m_run;
  st[wave * 128 + 64 + lane] = l_run;
  __syncthreads();
  float m_all = -INFINITY;
#pragma unroll
  for (int w = 0; w < NW; ++w) m_all = fmaxf(m_all, st[w * 128 + lane]);     // (equal in a lane and its partner)
  float f[NW], l_tot = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    f[w] = __builtin_amdgcn_exp2f(st[w * 128 + lane] - m_all);               // a wave without keys: 2^-inf = 0
    l_tot += (st[w * 128 + 64 + lane] + st[w * 128 + 64 + (lane ^ 32)]) * f[w];
  }
  const int q = q0 + (lane & 31);
  const size_t row = (size_t)b * a.q_len + q;
  const size_t rows = (size_t)a.batch * a.q_len;
  const float inv = 1.f / l_tot;
#pragma unroll
  for (int c = 0; c < EC; ++c) {
#pragma unroll
    for (int r = 0; r < 16; ++r) xa[(wave * 16 + r) * 64 + lane] = acc[c][r];
    __syncthreads();
    if (wave < 4) {
      float o4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int e = 0; e < 4; ++e) o4[e] += xa[(w * 16 + 4 * wave + e) * 64 + lane] * f[w];
      const int ch = 32 * c + 8 * wave + 4 * hi;
      if (q < a.q_len && ch < E) {
        if (a.part_o) {
          float *po = a.part_o + ((size_t)blockIdx.z * rows + row) * E + ch;
          qkv_store4(po, o4[0], o4[1], o4[2], o4[3]);
        } else {
          T *o = static_cast<T *>(a.out) + row * E + ch;
          qkv_store4(o, o4[0] * inv, o4[1] * inv, o4[2] * inv, o4[3] * inv);
        }
      }
    }
    if (c + 1 < EC) __syncthreads();
  }
  if (a.part_o && wave == 0 && hi == 0 && q < a.q_len)
    *reinterpret_cast<float2 *>(a.part_ml + ((size_t)blockIdx.z * rows + row) * 2) = make_float2(m_all, l_tot);
}

template <int E, int NW>
constexpr size_t qkv_f16_lds() {
  return std::max((size_t)NW * 32 * (64 * ((E + 31) / 32) + 16), (size_t)NW * 18 * 64 * sizeof(float));
}

// one tile's operands of a wave: the K fragment (row = key lane & 31, clamped into the sequence: those scores are
// masked) and its share of the V tile (16-byte chunks; rows past kv_len are zero)
template <int E>
__device__ __forceinline__ void qkv_f16_load_tile(const __half *kp, const __half *vp, int kv_len, int k0, int lane,
                                                  f16x8_t (&kf)[E / 16], uint4 (&vr)[E / 16]) {
  const int key = min(k0 + (lane & 31), kv_len - 1), hi = lane >> 5;
#pragma unroll
  for (int t = 0; t < E / 16; ++t)
    kf[t] = *reinterpret_cast<const f16x8_t *>(kp + (size_t)key * E + 16 * t + 8 * hi);
#pragma unroll
  for (int j = 0; j < E / 16; ++j) {
    const int idx = lane + 64 * j, r = idx / (E / 8), c = idx % (E / 8);
    vr[j] = k0 + r < kv_len ? *reinterpret_cast<const uint4 *>(vp + (size_t)(k0 + r) * E + 8 * c)
                            : make_uint4(0, 0, 0, 0);
  }
}

template <int E, int NW>
__global__ __launch_bounds__(64 * NW) void qkv_f16_kernel(QkvArgs a) {
  constexpr int ET = E / 16, EC = (E + 31) / 32;
  constexpr int kVRow = 64 * EC + 16;     // LDS bytes per V row: channels padded to 32 EC (never stored), + 16 so the
                                          // two lane halves (keys 4 apart) read different banks
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5, l32 = lane & 31;
  const int qt = (a.q_len + 31) >> 5;
  const int b = blockIdx.x / qt, q0 = (blockIdx.x - b * qt) * 32;
  const __half *qp = static_cast<const __half *>(a.q) + (size_t)b * a.q_len * E;
  const __half *kp = static_cast<const __half *>(a.k) + (size_t)b * a.kv_len * E;
  const __half *vp = static_cast<const __half *>(a.v) + (size_t)b * a.kv_len * E;
  const int ntiles = (a.kv_len + 31) >> 5;
  const int t_begin = blockIdx.z * a.tiles_per_split, t_end = min(t_begin + a.tiles_per_split, ntiles);

  // Q fragment (B operand: column = query lane & 31, k = channels 16 t + 8 hi ..); queries past q_len are clamped
  const int qi = min(q0 + l32, a.q_len - 1);
  f16x8_t qf[ET];
#pragma unroll
  for (int t = 0; t < ET; ++t) qf[t] = *reinterpret_cast<const f16x8_t *>(qp + (size_t)qi * E + 16 * t + 8 * hi);

  char *vs = smem + wave * 32 * kVRow;
  f32x16_t acc[EC];
#pragma unroll
  for (int c = 0; c < EC; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  f16x8_t kf[ET];
  uint4 vr[ET];
  int tile = t_begin + wave;
  if (tile < t_end) qkv_f16_load_tile<E>(kp, vp, a.kv_len, tile * 32, lane, kf, vr);
  for (; tile < t_end; tile += NW) {
    const int k0 = tile * 32;
#pragma unroll
    for (int j = 0; j < ET; ++j) {
      const int idx = lane + 64 * j, r = idx / (E / 8), c = idx % (E / 8);
      *reinterpret_cast<uint4 *>(vs + r * kVRow + c * 16) = vr[j];
    }
    f16x8_t kc[ET];
#pragma unroll
    for (int t = 0; t < ET; ++t) kc[t] = kf[t];
    if (tile + NW < t_end) qkv_f16_load_tile<E>(kp, vp, a.kv_len, (tile + NW) * 32, lane, kf, vr);   // in flight

    f32x16_t s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int t = 0; t < ET; ++t) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kc[t], qf[t], s, 0, 0, 0);
    float p[16];
    const float alpha = qkv_online_softmax(s, p, m_run, l_run, k0, a.kv_len, hi, a.scale_log2e);
#pragma unroll
    for (int c = 0; c < EC; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][r] *= alpha;
    // O^T += V^T P^T, 16 keys per instruction: k index 8 hi + i  <->  key (i & 3) + 8 (i >> 2) + 4 hi + 16 u
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      f16x8_t pf;
#pragma unroll
      for (int i = 0; i < 8; ++i) pf[i] = (_Float16)p[8 * u + i];
#pragma unroll
      for (int c = 0; c < EC; ++c) {
        f16x8_t vf;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int key = (i & 3) + 8 * (i >> 2) + 4 * hi + 16 * u;
          vf[i] = *reinterpret_cast<const _Float16 *>(vs + key * kVRow + (32 * c + l32) * 2);
        }
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, acc[c], 0, 0, 0);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  qkv_block_merge<E, NW, __half>(a, smem, acc, m_run, l_run, b, q0);
}

constexpr int kQkvF32Waves = 4;

// fp32: k = 2 channels per instruction, one per lane half; lane half hi walks channels hi * E / 2 + j (any bijection of
// the channels does for a dot product, and this one makes a lane's Q and K elements contiguous 16-byte loads)
template <int E>
__global__ __launch_bounds__(64 * kQkvF32Waves) void qkv_f32_kernel(QkvArgs a) {
  constexpr int NW = kQkvF32Waves, EH = E / 2, EC = (E + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5, l32 = lane & 31;
  const int qt = (a.q_len + 31) >> 5;
  const int b = blockIdx.x / qt, q0 = (blockIdx.x - b * qt) * 32;
  const float *qp = static_cast<const float *>(a.q) + (size_t)b * a.q_len * E;
  const float *kp = static_cast<const float *>(a.k) + (size_t)b * a.kv_len * E;
  const float *vp = static_cast<const float *>(a.v) + (size_t)b * a.kv_len * E;
  const int ntiles = (a.kv_len + 31) >> 5;
  const int t_begin = blockIdx.z * a.tiles_per_split, t_end = min(t_begin + a.tiles_per_split, ntiles);

  const int qi = min(q0 + l32, a.q_len - 1);
  float qv[EH];
#pragma unroll
  for (int j = 0; j < EH / 4; ++j) {
    const float4 x = *reinterpret_cast<const float4 *>(qp + (size_t)qi * E + hi * EH + 4 * j);
    qv[4 * j] = x.x, qv[4 * j + 1] = x.y, qv[4 * j + 2] = x.z, qv[4 * j + 3] = x.w;
  }
  f32x16_t acc[EC];
#pragma unroll
  for (int c = 0; c < EC; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  for (int tile = t_begin + wave; tile < t_end; tile += NW) {
    const int k0 = tile * 32;
    const int key = min(k0 + l32, a.kv_len - 1);
    float kv[EH];
#pragma unroll
    for (int j = 0; j < EH / 4; ++j) {
      const float4 x = *reinterpret_cast<const float4 *>(kp + (size_t)key * E + hi * EH + 4 * j);
      kv[4 * j] = x.x, kv[4 * j + 1] = x.y, kv[4 * j + 2] = x.z, kv[4 * j + 3] = x.w;
    }
    // V^T operand of step r: V[key (r & 3) + 8 (r >> 2) + 4 hi][32 c + lane & 31]; zero past the sequence / channels
    float vv[EC][16];
#pragma unroll
    for (int c = 0; c < EC; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kr = k0 + (r & 3) + 8 * (r >> 2) + 4 * hi, ch = 32 * c + l32;
        vv[c][r] = (kr < a.kv_len && ch < E) ? vp[(size_t)kr * E + ch] : 0.f;
      }
    f32x16_t s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int j = 0; j < EH; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[j], qv[j], s, 0, 0, 0);
    float p[16];
    const float alpha = qkv_online_softmax(s, p, m_run, l_run, k0, a.kv_len, hi, a.scale_log2e);
#pragma unroll
    for (int c = 0; c < EC; ++c) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][r] *= alpha;
      // step r: k = hi <-> key (r & 3) + 8 (r >> 2) + 4 hi, whose probability is this lane's own register r
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv[c][r], p[r], acc[c], 0, 0, 0);
    }
  }
  qkv_block_merge<E, NW, float>(a, smem, acc, m_run, l_run, b, q0);
}

// out[row, 4 channels] = sum_s part_o[s] 2^(m_s - m) / sum_s l_s 2^(m_s - m), splits in ascending order
template <typename T>
__global__ __launch_bounds__(256) void qkv_merge_kernel(const float *__restrict__ part_o,
                                                        const float *__restrict__ part_ml, T *__restrict__ out,
                                                        size_t rows, int E, int nsplit) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int e4 = E >> 2;
  if (idx >= rows * e4) return;
  const size_t row = idx / e4;
  const int ch = 4 * (int)(idx - row * e4);
  float m = -INFINITY;
  for (int s = 0; s < nsplit; ++s) m = fmaxf(m, part_ml[(s * rows + row) * 2]);
  float l = 0.f, o[4] = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < nsplit; ++s) {
    const float2 ml = *reinterpret_cast<const float2 *>(part_ml + (s * rows + row) * 2);
    const float f = __builtin_amdgcn_exp2f(ml.x - m);
    l += ml.y * f;
    const float4 x = *reinterpret_cast<const float4 *>(part_o + (s * rows + row) * E + ch);
    o[0] += x.x * f, o[1] += x.y * f, o[2] += x.z * f, o[3] += x.w * f;
  }
  const float inv = 1.f / l;
  qkv_store4(out + row * E + ch, o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv);
}

int qkv_waves(int dtype, int E) { return dtype == BEVOPS_F16 && E <= 64 ? 8 : 4; }

struct QkvPlan {
  int qt, ntiles, nsplit, tiles_per_split;
};

// Key split: only when the (query tile, batch) blocks fill less than three quarters of the CUs; then aim at two blocks
// per CU with at least two key tiles per wave in every split.  A pure function of the shape (so is the workspace size).
QkvPlan qkv_plan(int dtype, int batch, int q_len, int kv_len, int E) {
  QkvPlan p;
  p.qt = (q_len + 31) / 32;
  p.ntiles = (kv_len + 31) / 32;
  const long long blocks = (long long)batch * p.qt;
  long long ns = 1;
  if (blocks < 3 * kQkvCUs / 4) {
    const long long want = (2 * kQkvCUs + blocks - 1) / blocks;
    const long long most = p.ntiles / (2 * qkv_waves(dtype, E));
    ns = std::max(1LL, std::min(want, most));
  }
  p.tiles_per_split = (int)((p.ntiles + ns - 1) / ns);
  p.nsplit = (p.ntiles + p.tiles_per_split - 1) / p.tiles_per_split;
  return p;
}

bool qkv_dim_ok(int E) { return E >= kQkvMinE && E <= kQkvMaxE && E % 16 == 0; }

template <int E>
int qkv_launch(int dtype, const QkvArgs &a, const QkvPlan &p, hipStream_t stream) {
  const dim3 grid((unsigned)((long long)a.batch * p.qt), 1, (unsigned)p.nsplit);
  if (dtype == BEVOPS_F16) {
    constexpr int NW = E <= 64 ? 8 : 4;
    constexpr size_t lds = qkv_f16_lds<E, NW>();
    if (!ensure_dynamic_lds<qkv_f16_kernel<E, NW>>(lds)) return BEVOPS_FAILURE;
    hipLaunchKernelGGL((qkv_f16_kernel<E, NW>), grid, dim3(64 * NW), lds, stream, a);
  } else {
    constexpr size_t lds = (size_t)kQkvF32Waves * 18 * 64 * sizeof(float);
    hipLaunchKernelGGL((qkv_f32_kernel<E>), grid, dim3(64 * kQkvF32Waves), lds, stream, a);
  }
  if (p.nsplit > 1) {
    const size_t rows = (size_t)a.batch * a.q_len, n = rows * (E / 4);
    const dim3 mgrid((unsigned)((n + 255) / 256));
    if (dtype == BEVOPS_F16)
      hipLaunchKernelGGL(qkv_merge_kernel<__half>, mgrid, dim3(256), 0, stream, a.part_o, a.part_ml,
                         static_cast<__half *>(a.out), rows, E, p.nsplit);
    else
      hipLaunchKernelGGL(qkv_merge_kernel<float>, mgrid, dim3(256), 0, stream, a.part_o, a.part_ml,
                         static_cast<float *>(a.out), rows, E, p.nsplit);
  }
  return launch_status();
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" size_t bevops_qkv_workspace_size(int dtype, int batch, int q_len, int kv_len, int embed_dim) {
  if ((dtype != BEVOPS_F32 && dtype != BEVOPS_F16) || batch <= 0 || q_len <= 0 || kv_len <= 0 ||
      !qkv_dim_ok(embed_dim))
    return 0;
  const QkvPlan p = qkv_plan(dtype, batch, q_len, kv_len, embed_dim);
  if (p.nsplit <= 1) return 0;
  // partial outputs [nsplit][B Lq][E], then (maximum, sum) [nsplit][B Lq][2]; fp32
  return (size_t)p.nsplit * batch * q_len * (embed_dim + 2) * sizeof(float);
}

extern "C" int bevops_qkv_forward(int dtype, const void *query, const void *key, const void *value, void *output,
                                  int batch, int q_len, int kv_len, int embed_dim, float scale_q, float scale_k,
                                  float scale_v, float scale_o, void *workspace, size_t workspace_bytes,
                                  void *stream) {
  (void)scale_q, (void)scale_k, (void)scale_v, (void)scale_o;   // INT8 only (not supported yet)
  if (!query || !key || !value || !output || batch <= 0 || q_len <= 0 || kv_len <= 0 || embed_dim <= 0)
    return BEVOPS_BAD_PARAM;
  if (dtype != BEVOPS_F32 && dtype != BEVOPS_F16) return BEVOPS_NOT_SUPPORTED;
  if (!qkv_dim_ok(embed_dim)) return BEVOPS_NOT_SUPPORTED;
  if (!aligned16(query) || !aligned16(key) || !aligned16(value) || !aligned16(output)) return BEVOPS_BAD_PARAM;
  const QkvPlan p = qkv_plan(dtype, batch, q_len, kv_len, embed_dim);
  if ((long long)batch * p.qt > INT_MAX) return BEVOPS_NOT_SUPPORTED;
  const size_t need = bevops_qkv_workspace_size(dtype, batch, q_len, kv_len, embed_dim);
  if (need && (!workspace || workspace_bytes < need || !aligned16(workspace))) return BEVOPS_BAD_PARAM;
  QkvArgs a;
  a.q = query, a.k = key, a.v = value, a.out = output;
  a.part_o = need ? static_cast<float *>(workspace) : nullptr;
  a.part_ml = need ? a.part_o + (size_t)p.nsplit * batch * q_len * embed_dim : nullptr;
  a.batch = batch, a.q_len = q_len, a.kv_len = kv_len, a.tiles_per_split = p.tiles_per_split;
  a.scale_log2e = 1.4426950408889634f / sqrtf((float)embed_dim);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  switch (embed_dim) {
    case 16: return qkv_launch<16>(dtype, a, p, st);
    case 32: return qkv_launch<32>(dtype, a, p, st);
    case 48: return qkv_launch<48>(dtype, a, p, st);
    case 64: return qkv_launch<64>(dtype, a, p, st);
    case 80: return qkv_launch<80>(dtype, a, p, st);
    case 96: return qkv_launch<96>(dtype, a, p, st);
    case 112: return qkv_launch<112>(dtype, a, p, st);
    case 128: return qkv_launch<128>(dtype, a, p, st);
    default: return BEVOPS_NOT_SUPPORTED;
  }
}
