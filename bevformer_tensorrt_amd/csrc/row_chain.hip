// A CHAIN of dense layers over the same FEW rows as one launch (the decoder's 900 object queries: a layer's output_proj /
// FFN / branch layers, the six levels' classification branches -- design/model.md "Row chains"):
//     y_s = act_s( LayerNorm_s( in_s @ W_s.T + bias_s + identity_s ) ),   s = 0 .. S - 1,  fp16 in / out, fp32 sums,
// where in_s is x or the output of an earlier stage and identity_s a tensor or the input rows of an earlier stage.  Such
// a chain has a microsecond of matrix work and a megabyte of weights; per-layer launches spend their time on the kernel
// boundaries between them.  Rows are independent, so a block owns 16 rows and walks the whole chain:
//   * the row tile of every stage sits in LDS as fp16 (one region per stage output that a later stage reads, rows padded
//     by 16 bytes), with every stage's bias / gamma / beta behind them -- all in ONE dynamic array, filled by one round
//     of loads at the start of the block;
//   * kRcWaves waves, wave w owns the 16-column tiles w, w + kRcWaves, ... of a stage.  Weights go from global memory
//     straight into the operand registers of v_mfma_f32_16x16x32_f16 (every weight element is used once per block: no
//     LDS staging; `packed` weights lie in that order, one contiguous kilobyte per request), in units of 8 k-steps,
//     kRcDepth units requested ahead of the one being multiplied.  The unit loop has NO conditional
//     memory operation (units past the wave's last and k-steps past K are requested beyond the buffer's range: zeros,
//     multiplied against zero-filled LDS columns), so the compiler counts the outstanding requests exactly;
//   * operand A = weight rows, B = activation rows: a lane ends with 4 consecutive columns of one row -- bias, identity,
//     (LayerNorm,) activation in fp32, ONE rounding, an 8-byte store to LDS and / or the stage's destinations;
//   * LayerNorm: the unrounded fp32 rows meet in an LDS scratch, kRcLnLanes threads per row take mean and centred
//     squares in fp32 (fixed order: ascending columns per thread, then a butterfly over the row's lanes) -- ts_ln_row's
//     arithmetic on the unrounded row.
// A row's result depends on its own operands only: not on M, the block index or the CU count.  No atomics, no
// cross-block hand-off.  GROUPS > 1: block (g, tile) works on rows g * M .. of every row operand with the weights /
// bias / gamma / beta of group g from stacked tensors.
#include "gemm_host.h"

namespace bevops {
namespace {

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

// Waves per block and units requested ahead, measured per site under graph replay (design/model.md "Row chains"): a wave
// is bound by its own chain of dependent steps (request, eight dependent matrix instructions, epilogue), not by
// bandwidth, so more and shorter waves win -- 4 x 4: 56 us for the decoder tail, 8 x 2: 39, 8 x 1: 37, 16 x 1: 31.
#ifndef RC_WAVES
#define RC_WAVES 16
#endif
#ifndef RC_DEPTH
#define RC_DEPTH 1
#endif
constexpr int kRcRows = 16, kRcWaves = RC_WAVES, kRcThreads = 64 * kRcWaves, kRcDepth = RC_DEPTH, kRcUnit = 8;   // unit: 8 k-steps of 32
constexpr int kRcLnLanes = kRcThreads / kRcRows;                 // threads per row of the norm pass
constexpr int kRcUnitK = kRcUnit * 32;
constexpr int kRcMaxStages = 8, kRcMaxK = 768, kRcMaxN = 768, kRcPad = 8;
constexpr int kRcXLoads = (kRcRows * kRcMaxK / 8 + kRcThreads - 1) / kRcThreads;    // 16-byte pieces of the x tile per thread
constexpr int kRcParLoads = (kRcMaxN + kRcThreads - 1) / kRcThreads;                // elements of a bias / gamma / beta per thread
constexpr int kRcMaxTiles = (kRcMaxN / 16 + kRcWaves - 1) / kRcWaves;             // 16-column tiles of a stage per wave
constexpr size_t kRcMaxLds = 160 * 1024;

struct RcStage {
  const __half *w, *bias, *gamma, *beta, *res;
  __half *out[2];
  int pitch[2], c0[2], c1[2];
  int K, N, act, norm, ndst, packed;
  // LDS: byte offset and row stride (elements) of the input rows, the output rows (offset -1: nobody reads them) and an
  // identity taken from LDS (offset -1: none, or the tensor `res`); byte offset of bias | gamma | beta (N4 halfs each)
  int in_off, in_stride, out_off, out_stride, res_off, res_stride, par_off;
  unsigned res_bytes;
  int res_pitch;
  float eps;
};

struct RcArgs {
  const __half *x;
  unsigned x_bytes;
  int x_pitch, M, tiles_m, nstages, ln_off, ln_stride, zero_bytes;   // zero_bytes: row regions to clear first (0: none padded)
  RcStage s[kRcMaxStages];
};

// act, one rounding, then the stage's LDS rows and its destinations: columns n .. n + 3 of tile row `row`
__device__ __forceinline__ void rc_emit(const RcStage &st, char *lds, long long grow, int row, bool m_ok, int n, f32x4 v) {
  if (st.act) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
  }
  const u32x2 q = {pack_h2(v[0], v[1]), pack_h2(v[2], v[3])};
  if (st.out_off >= 0)   // (a stage that is read has N % 32 == 0: the four columns exist)
    *reinterpret_cast<u32x2 *>(lds + st.out_off + ((size_t)row * st.out_stride + n) * 2) = q;
  if (!m_ok) return;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    if (d >= st.ndst || n < st.c0[d] || n >= st.c1[d]) continue;
    __half *o = st.out[d] + grow * st.pitch[d] + (n - st.c0[d]);
    if (n + 3 < st.c1[d] && (st.pitch[d] & 3) == 0) {
      *reinterpret_cast<u32x2 *>(o) = q;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (n + i < st.c1[d]) o[i] = __ushort_as_half((unsigned short)((i & 1 ? q[i >> 1] >> 16 : q[i >> 1]) & 0xffffu));
    }
  }
}

__device__ __forceinline__ float rc_row_sum(float v) {   // the lanes of a row: every lane ends with the same sum
#pragma unroll
  for (int k = 1; k < kRcLnLanes; k <<= 1) v += __shfl_xor(v, k, kRcLnLanes);
  return v;
}

__device__ __forceinline__ f32x4 rc_h4(u32x2 q) { return f32x4{h2f_lo(q[0]), h2f_hi(q[0]), h2f_lo(q[1]), h2f_hi(q[1])}; }

__global__ __launch_bounds__(kRcThreads) void row_chain_f16_kernel(const RcArgs p) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = (int)blockIdx.x / p.tiles_m, m0 = ((int)blockIdx.x % p.tiles_m) * kRcRows;
  const long long grow0 = (long long)g * p.M + m0;   // first row of the tile in every row operand
  const int l15 = lane & 15, kofs = 8 * (lane >> 4);

  {  // one round of loads: the x tile (stage 0's input region, offset 0; rows past M as zeros) and every stage's parameters
    const int K0 = p.s[0].K, per_row = K0 / 8;
    // (every request goes through a buffer descriptor and is unconditional -- what lies outside reads as zero -- so
    // all of them are in flight before the first is waited for)
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<__half *>(p.x), 0, p.x_bytes, 0x00020000);
    u32x4 xr[kRcXLoads];
#pragma unroll
    for (int i = 0; i < kRcXLoads; ++i) {
      const int id = tid + i * kRcThreads, r = id / per_row, c = (id % per_row) * 8;
      const bool ok = r < kRcRows && m0 + r < p.M;
      xr[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)(ok ? (unsigned)(((grow0 + r) * p.x_pitch + c) * 2) : kGemmOob), 0, 0);
    }
    unsigned short pr[kRcMaxStages][3][kRcParLoads];
#pragma unroll
    for (int s = 0; s < kRcMaxStages; ++s)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const __half *src = a == 0 ? p.s[s].bias : a == 1 ? p.s[s].gamma : p.s[s].beta;
        const int n = s < p.nstages ? p.s[s].N : 0;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<__half *>(src), 0, src ? (unsigned)((g + 1) * n * 2) : 0u, 0x00020000);
#pragma unroll
        for (int i = 0; i < kRcParLoads; ++i) {
          const int id = tid + i * kRcThreads;
          pr[s][a][i] = __builtin_amdgcn_raw_buffer_load_b16(rs, (int)(id < n ? (unsigned)((g * n + id) * 2) : kGemmOob), 0, 0);
        }
      }
    if (p.zero_bytes) {   // a K that is no multiple of a unit: the columns behind it are multiplied (against zeros)
      for (int i = tid * 16; i < p.zero_bytes; i += kRcThreads * 16) *reinterpret_cast<uint4 *>(lds + i) = make_uint4(0u, 0u, 0u, 0u);
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < kRcXLoads; ++i) {
      const int id = tid + i * kRcThreads, r = id / per_row, c = (id % per_row) * 8;
      if (r < kRcRows) *reinterpret_cast<u32x4 *>(lds + ((size_t)r * p.s[0].in_stride + c) * 2) = xr[i];
    }
#pragma unroll
    for (int s = 0; s < kRcMaxStages; ++s)
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int i = 0; i < kRcParLoads; ++i) {
          const int id = tid + i * kRcThreads;
          if (s < p.nstages && id < p.s[s].N)
            *reinterpret_cast<unsigned short *>(lds + p.s[s].par_off + ((size_t)a * ((p.s[s].N + 3) & ~3) + id) * 2) = pr[s][a][i];
        }
  }

  for (int s = 0; s < p.nstages; ++s) {
    const RcStage &st = p.s[s];
    const int K = st.K, N = st.N, N4 = (N + 3) & ~3, ksteps = K / 32;
    const int chunks = (ksteps + kRcUnit - 1) / kRcUnit;
    const int ntiles = (N + 15) / 16;
    const int my_tiles = wave < ntiles ? (ntiles - wave + kRcWaves - 1) / kRcWaves : 0;
    const int units = my_tiles * chunks;
    // packed weights hold whole 16-row tiles in fragment order (rows past N are zeros in memory)
    const size_t w_elems = (size_t)(st.packed ? ntiles * 16 : N) * K;
    const __half *wg = st.w + (size_t)g * w_elems;
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<__half *>(wg), 0, (unsigned)(w_elems * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_r = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<__half *>(st.res), 0, st.res_bytes, 0x00020000);   // (no tensor identity: 0 bytes, every read a zero)
    const bool m_ok = m0 + l15 < p.M;
    const char *in_rows = lds + st.in_off + ((size_t)l15 * st.in_stride + kofs) * 2;
    const unsigned res_row = (unsigned)((grow0 + l15) * st.res_pitch * 2);
    // the identity rows do not depend on the sums: this lane's 4 columns of every tile of the wave, requested first
    u32x2 res_t[kRcMaxTiles];
#pragma unroll
    for (int t = 0; t < kRcMaxTiles; ++t) {
      const int n = (wave + kRcWaves * t) * 16 + 4 * (lane >> 4);
      res_t[t] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(
          rs_r, (int)(m_ok && n < N ? res_row + (unsigned)n * 2 : kGemmOob), 0, 0));
    }
    __builtin_amdgcn_sched_barrier(0);

    // the weight fragments of unit (tile j of this wave, chunk c): rows past N, k-steps past K, tiles past the wave's
    // last read as zero
    auto load_unit = [&](u32x4(&f)[kRcUnit], int j, int c) {
      const int tile = wave + kRcWaves * j, n = tile * 16 + l15;
      // row-major: 64 bytes of each of 16 rows per request; packed: the request's 1 KB is contiguous (k-step s of tile t
      // at ((t ksteps + s) 64 + lane) 16 bytes), the same values in the same registers
      const unsigned base = st.packed ? (unsigned)((((size_t)tile * ksteps + c * kRcUnit) * 64 + lane) * 16)
                                      : (unsigned)(((size_t)n * K + c * kRcUnitK + kofs) * 2);
      const unsigned step = st.packed ? 1024u : 64u;
      const bool n_ok = st.packed ? tile < ntiles : n < N;
#pragma unroll
      for (int i = 0; i < kRcUnit; ++i) {
        const bool ok = n_ok && c * kRcUnit + i < ksteps;
        f[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, (int)(ok ? base + i * step : kGemmOob), 0, 0);
      }
    };

    u32x4 wf[kRcDepth][kRcUnit];
    int pj = 0, pc = 0;   // the next unit to request
#pragma unroll
    for (int d = 0; d < kRcDepth; ++d) {
      load_unit(wf[d], pj, pc);
      if (++pc == chunks) { pc = 0; ++pj; }
      __builtin_amdgcn_sched_barrier(0);   // (requests stay in the order they are consumed in)
    }
    __syncthreads();   // the rows this stage reads are in LDS; the scratch of an earlier norm is free
    int cj = 0, cc = 0;   // the unit being multiplied
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int u0 = 0; u0 < units; u0 += kRcDepth) {
#pragma unroll
      for (int d = 0; d < kRcDepth; ++d) {
        const int n = (wave + kRcWaves * cj) * 16 + 4 * (lane >> 4);   // this lane's 4 columns of the tile
        if (cc == 0) acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < kRcUnit; ++i) {
          const u32x4 b = *reinterpret_cast<const u32x4 *>(in_rows + (size_t)(cc * kRcUnit + i) * 64);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, wf[d][i]),
                                                       __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        load_unit(wf[d], pj, pc);
        if (++pc == chunks) { pc = 0; ++pj; }
        __builtin_amdgcn_sched_barrier(0);
        if (cc == chunks - 1 && cj < my_tiles && n < N) {
          f32x4 v = acc + rc_h4(*reinterpret_cast<const u32x2 *>(lds + st.par_off + (size_t)n * 2));   // (no bias: zeros)
          if (st.res_off >= 0)   // identity: the input rows of an earlier stage (width N)
            v += rc_h4(*reinterpret_cast<const u32x2 *>(lds + st.res_off + ((size_t)l15 * st.res_stride + n) * 2));
          else {
            u32x2 rres = res_t[0];
#pragma unroll
            for (int t = 1; t < kRcMaxTiles; ++t) rres = cj == t ? res_t[t] : rres;
            v += rc_h4(rres);
          }
          if (st.norm)
            *reinterpret_cast<f32x4 *>(lds + p.ln_off + ((size_t)l15 * p.ln_stride + n) * 4) = v;
          else
            rc_emit(st, lds, grow0 + l15, l15, m_ok, n, v);
        }
        if (++cc == chunks) { cc = 0; ++cj; }
      }
    }

    if (st.norm) {
      __syncthreads();   // the unrounded rows are in the scratch
      const int row = tid / kRcLnLanes, j = tid % kRcLnLanes;
      const float *srow = reinterpret_cast<const float *>(lds + p.ln_off) + (size_t)row * p.ln_stride;
      const float inv_n = 1.f / (float)N;
      float sum = 0.f;
      for (int c = 4 * j; c < N; c += 4 * kRcLnLanes) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(srow + c);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c + i < N) sum += v[i];
      }
      const float mean = rc_row_sum(sum) * inv_n;
      float sq = 0.f;
      for (int c = 4 * j; c < N; c += 4 * kRcLnLanes) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(srow + c);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c + i < N) sq = fmaf(v[i] - mean, v[i] - mean, sq);
      }
      const float rstd = rsqrtf(rc_row_sum(sq) * inv_n + st.eps);
      const char *gamma = lds + st.par_off + (size_t)N4 * 2, *beta = gamma + (size_t)N4 * 2;
      for (int c = 4 * j; c < N; c += 4 * kRcLnLanes) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(srow + c);
        const f32x4 gg = rc_h4(*reinterpret_cast<const u32x2 *>(gamma + (size_t)c * 2));
        const f32x4 bb = rc_h4(*reinterpret_cast<const u32x2 *>(beta + (size_t)c * 2));
        f32x4 y = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c + i < N) y[i] = fmaf((v[i] - mean) * rstd, gg[i], bb[i]);
        rc_emit(st, lds, grow0 + row, row, m0 + row < p.M, c, y);
      }
    }
  }
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_row_chain_f16(const void *x, long long x_pitch, const bevops_chain_stage *stages, int num_stages,
                                    long long M, int groups, void *stream) {
  if (!x || !stages || num_stages <= 0 || M < 0 || groups <= 0 || x_pitch <= 0) return BEVOPS_BAD_PARAM;
  if (num_stages > kRcMaxStages) return BEVOPS_NOT_SUPPORTED;
  RcArgs a{};
  // src[s]: the stage whose output stage s reads (-1: x); read[s + 1]: somebody reads the output of stage s from LDS
  int src[kRcMaxStages];
  bool read[kRcMaxStages + 1] = {};
  for (int s = 0; s < num_stages; ++s) {
    const bevops_chain_stage &e = stages[s];
    if (!e.weight || e.K <= 0 || e.N <= 0 || e.input >= s || e.input < -1 || e.res_stage > s || e.res_stage < -1 ||
        (e.res && e.res_stage >= 0) || (e.norm && (!e.gamma || !e.beta || !(e.eps >= 0.f))) || e.num_dst < 0 || e.num_dst > 2 ||
        (e.act != 0 && e.act != 1))
      return BEVOPS_BAD_PARAM;
    if (e.K % 32 != 0 || e.K > kRcMaxK || e.N > kRcMaxN) return BEVOPS_NOT_SUPPORTED;
    if (misaligned(e.weight, 15u) || (e.bias && misaligned(e.bias, 15u)) || (e.res && misaligned(e.res, 15u)) ||
        (e.norm && (misaligned(e.gamma, 15u) || misaligned(e.beta, 15u))))
      return BEVOPS_NOT_SUPPORTED;
    src[s] = e.input < 0 ? s - 1 : e.input;
    const int k_in = src[s] < 0 ? e.K : stages[src[s]].N;
    if (k_in != e.K) return BEVOPS_BAD_PARAM;
    read[src[s] + 1] = true;
    if (e.res_stage >= 0) {
      const int r = src[e.res_stage];                  // identity = the input rows of stage res_stage
      if ((r < 0 ? stages[0].K : stages[r].N) != e.N) return BEVOPS_BAD_PARAM;
      read[r + 1] = true;
    }
    if (e.res) {   // read 8 bytes at a time through a 32-bit byte offset
      if (e.res_pitch < e.N || e.res_pitch > 0x7fffffffLL) return BEVOPS_BAD_PARAM;
      if (e.N % 4 != 0 || e.res_pitch % 4 != 0 || gemm_over_limit((unsigned long long)M * groups, (int)e.res_pitch, 2))
        return BEVOPS_NOT_SUPPORTED;
    }
    for (int d = 0; d < e.num_dst; ++d) {
      const bevops_chain_dst &o = e.dst[d];
      if (!o.out || o.col_begin < 0 || o.col_end > e.N || o.col_end <= o.col_begin || o.col_begin % 8 != 0 ||
          o.pitch < o.col_end - o.col_begin || o.pitch > 0x7fffffffLL || (d == 1 && o.col_begin < e.dst[0].col_end))
        return BEVOPS_BAD_PARAM;
      if (misaligned(o.out, 15u)) return BEVOPS_NOT_SUPPORTED;
    }
  }
  if (misaligned(x, 15u) || x_pitch % 8 != 0 || x_pitch < stages[0].K || x_pitch > 0x7fffffffLL ||
      gemm_over_limit((unsigned long long)M * groups, (int)x_pitch, 2))
    return BEVOPS_NOT_SUPPORTED;
  const long long tiles_m = (M + kRcRows - 1) / kRcRows;
  if (tiles_m * groups > 0x7fffffffLL || M * groups > 0x7fffffffLL) return BEVOPS_NOT_SUPPORTED;
  // LDS: x rows, then one region per stage output that is read (rows as wide as whole units of k), the norm scratch,
  // the stages' parameters
  size_t lds = 0;
  int off[kRcMaxStages + 1], stride[kRcMaxStages + 1];
  int ln_n = 0;
  bool padded = false;
  for (int s = -1; s < num_stages; ++s) {
    const int width = s < 0 ? stages[0].K : stages[s].N;
    off[s + 1] = -1;
    stride[s + 1] = 0;
    if (s >= 0 && stages[s].norm && width > ln_n) ln_n = width;
    if (!read[s + 1] && s >= 0) continue;
    const int wide = (width + kRcUnitK - 1) / kRcUnitK * kRcUnitK;
    padded = padded || wide != width;
    off[s + 1] = (int)lds;
    stride[s + 1] = wide + kRcPad;
    lds += (size_t)kRcRows * stride[s + 1] * 2;
    if (lds > kRcMaxLds) return BEVOPS_NOT_SUPPORTED;
  }
  a.zero_bytes = padded ? (int)lds : 0;
  a.ln_off = (int)lds;
  a.ln_stride = (ln_n + 3) / 4 * 4 + 4;
  if (ln_n) lds += (size_t)kRcRows * a.ln_stride * 4;
  int par[kRcMaxStages];
  for (int s = 0; s < num_stages; ++s) {
    par[s] = (int)lds;
    lds += (size_t)3 * ((stages[s].N + 3) / 4 * 4) * 2;
    lds = (lds + 15) / 16 * 16;
  }
  if (lds > kRcMaxLds) return BEVOPS_NOT_SUPPORTED;
  if (M == 0) return BEVOPS_SUCCESS;
  a.x = static_cast<const __half *>(x);
  a.x_pitch = (int)x_pitch;
  a.x_bytes = (unsigned)((unsigned long long)M * groups * x_pitch * 2);
  a.M = (int)M;
  a.tiles_m = (int)tiles_m;
  a.nstages = num_stages;
  for (int s = 0; s < num_stages; ++s) {
    const bevops_chain_stage &e = stages[s];
    RcStage &t = a.s[s];
    t.w = static_cast<const __half *>(e.weight);
    t.bias = static_cast<const __half *>(e.bias);
    t.gamma = e.norm ? static_cast<const __half *>(e.gamma) : nullptr;
    t.beta = e.norm ? static_cast<const __half *>(e.beta) : nullptr;
    t.res = static_cast<const __half *>(e.res);
    t.res_pitch = e.res ? (int)e.res_pitch : 0;
    t.res_bytes = e.res ? (unsigned)((unsigned long long)M * groups * e.res_pitch * 2) : 0u;
    t.packed = e.packed ? 1 : 0;
    t.K = e.K; t.N = e.N; t.act = e.act; t.norm = e.norm ? 1 : 0; t.ndst = e.num_dst; t.eps = e.eps;
    for (int d = 0; d < e.num_dst; ++d) {
      t.out[d] = static_cast<__half *>(e.dst[d].out);
      t.pitch[d] = (int)e.dst[d].pitch; t.c0[d] = e.dst[d].col_begin; t.c1[d] = e.dst[d].col_end;
    }
    t.in_off = off[src[s] + 1];
    t.in_stride = stride[src[s] + 1];
    t.out_off = off[s + 1];
    t.out_stride = stride[s + 1];
    t.res_off = e.res_stage >= 0 ? off[src[e.res_stage] + 1] : -1;
    t.res_stride = e.res_stage >= 0 ? stride[src[e.res_stage] + 1] : 0;
    t.par_off = par[s];
  }
  if (!ensure_dynamic_lds<row_chain_f16_kernel>(lds)) return BEVOPS_FAILURE;
  hipLaunchKernelGGL(row_chain_f16_kernel, dim3((unsigned)(tiles_m * groups)), dim3(kRcThreads), lds,
                     static_cast<hipStream_t>(stream), a);
  return launch_status();
}
