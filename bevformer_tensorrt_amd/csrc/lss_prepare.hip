// LSSViewTransformer.get_lidar_coor + voxel_pooling_prepare_v2 (third_party/bev_mmdet3d/models/necks/
// view_transformer.py:126-168, 239-312) on the device, with fixed-size outputs and no host round trip, so the
// index build of a BEVDet frame can follow the frame's calibration inside the frame's HIP graph.
//
// Index generation must be BIT-EXACT: the per-point arithmetic is the reference's op sequence in fp32, each product
// and sum rounded on its own, every 3x3 . 3x1 product summed in ascending k ((m0 p0 + m1 p1) + m2 p2):
//   p  = frustum - post_trans;  p = inverse(post_rots) . p;  p = (p.x p.z, p.y p.z, p.z);
//   p  = combine . p;  p += trans;  coor = bda . p
//   q  = (coor - lower) / interval  (IEEE division);  t = trunc(q)  (`.long()` truncates toward zero);
//   kept = 0 <= t < size on all three axes, tested on the truncated FLOAT (a NaN or a huge quotient drops the point
//   and never becomes an address);  cell = z (ny nx) + y nx + x.
// The small matrices (inverse(post_rots), combine = sensor2ego[:3,:3] @ inverse(cam2imgs), ...) come from the host.
//
// Order: kept points ascending by cell, inside a cell ascending by point index -- the STABLE sort, one valid reading
// of the reference's unspecified argsort order and the one rule that makes the arrays unique.  It is a
// least-significant-digit radix sort over the 32-bit key (cell; `cells` for a dropped point, so those end up behind
// every kept one) with 8-bit digits: per-block digit counts (LDS atomics: they decide counts only), a scan per digit
// row plus the scan of the 256 row sums, a scatter whose rank inside a block comes from wave ballots in element
// order.  Stable by construction, correct for any interval length up to all points in one cell; two passes at the
// 16 384 cells of BEVDet-R50.  Intervals are the run-length encoding of the sorted keys (flag, scan, ordered
// compaction).  ranks_feat and ranks_bev are derived after the sort.  Every launch is sized by host values only.
//
// A batch of samples (bevops_lss_voxel_prepare_batched) is the same launches over batch * n_cams cameras: sample b
// reads row b of calib (its own cameras and bda), the key is b * cells + cell (batch * cells for a dropped point), and
// the digit count follows batch * cells.  At batch = 1 that is the single-sample build, launch for launch.
#include <math.h>

#include "common.h"
#include "lss_pos.h"

namespace bevops {
namespace {

constexpr int kLssBlock = 256;                 // 4 waves
constexpr int kLssItems = 8;                   // chunks of kLssBlock elements per block
constexpr int kLssTile = kLssBlock * kLssItems;
constexpr int kLssWaves = kLssBlock / kWave;
constexpr int kLssScanBlock = 1024;
constexpr int kLssMaxPoints = 1 << 22;
constexpr int kLssMaxCells = 1 << 24;

struct LssGrid {
  float lower[3], interval[3], size[3];
  int nx, nxy, cells;
};

// calib: one row of calib_stride floats per sample; per camera 24 floats [inverse(post_rots) 9 | post_trans 3 |
// combine 9 | trans 3], then bda 9.  keys[i] = sample * g.cells + cell of point i, or `dropped` (= batch * g.cells) when
// it is dropped; hist[digit * nblocks + block] = digit-0 counts of the tile.
__global__ __launch_bounds__(kLssBlock) void lss_cell_kernel(
    const float *__restrict__ frustum, const float *__restrict__ calib, LssGrid g, int n_cams, int calib_stride,
    unsigned dropped, int dhw, int n, unsigned *__restrict__ keys, int *__restrict__ hist, int nblocks,
    float *__restrict__ coor_out) {
  __shared__ int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  for (int j = 0; j < kLssItems; ++j) {
    const int i = blockIdx.x * kLssTile + j * kLssBlock + threadIdx.x;
    if (i >= n) break;
    const int gcam = i / dhw;        // camera over the batch
    const int f = i - gcam * dhw;
    const int b = gcam / n_cams;
    const float *row = calib + (size_t)b * calib_stride;
    const float *c = row + (size_t)(gcam - b * n_cams) * 24;
    const float *bda = row + (size_t)n_cams * 24;
    float x = sub_rn(frustum[(size_t)f * 3 + 0], c[9]);
    float y = sub_rn(frustum[(size_t)f * 3 + 1], c[10]);
    float z = sub_rn(frustum[(size_t)f * 3 + 2], c[11]);
    lss_mat3(c, x, y, z);
    x = mul_rn(x, z);
    y = mul_rn(y, z);
    lss_mat3(c + 12, x, y, z);
    x = add_rn(x, c[21]);
    y = add_rn(y, c[22]);
    z = add_rn(z, c[23]);
    lss_mat3(bda, x, y, z);
    if (coor_out) {
      coor_out[(size_t)i * 3 + 0] = x;
      coor_out[(size_t)i * 3 + 1] = y;
      coor_out[(size_t)i * 3 + 2] = z;
    }
    const float tx = truncf(lss_div(sub_rn(x, g.lower[0]), g.interval[0]));
    const float ty = truncf(lss_div(sub_rn(y, g.lower[1]), g.interval[1]));
    const float tz = truncf(lss_div(sub_rn(z, g.lower[2]), g.interval[2]));
    const bool kept = tx >= 0.f && tx < g.size[0] && ty >= 0.f && ty < g.size[1] && tz >= 0.f && tz < g.size[2];
    const unsigned key =
        kept ? (unsigned)b * (unsigned)g.cells + (unsigned)((int)tz * g.nxy + (int)ty * g.nx + (int)tx) : dropped;
    keys[i] = key;
    atomicAdd(&h[key & 255u], 1);
  }
  __syncthreads();
  hist[threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(kLssBlock) void lss_hist_kernel(const unsigned *__restrict__ keys, int n, int shift,
                                                             int *__restrict__ hist, int nblocks) {
  __shared__ int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  for (int j = 0; j < kLssItems; ++j) {
    const int i = blockIdx.x * kLssTile + j * kLssBlock + threadIdx.x;
    if (i >= n) break;
    atomicAdd(&h[(keys[i] >> shift) & 255u], 1);
  }
  __syncthreads();
  hist[threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

__device__ __forceinline__ int lss_wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// exclusive scan over the block's threads; `ws` holds one int per wave; two barriers
template <int WAVES>
__device__ __forceinline__ int lss_block_excl_scan(int v, int *ws, int &total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int incl = lss_wave_incl_scan(v, lane);
  if (lane == kWave - 1) ws[wave] = incl;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int s = ws[w];
    if (w < wave) off += s;
    tot += s;
  }
  total = tot;
  __syncthreads();
  return off + incl - v;
}

// in-place exclusive scan of a[0..n) by ONE block (the run starts per tile: n = tiles); when total_out is not NULL,
// total_out[1] = the sum and total_out[0] = 0
__global__ __launch_bounds__(kLssScanBlock) void lss_scan_kernel(int *__restrict__ a, int n,
                                                                 int *__restrict__ total_out) {
  __shared__ int ws[kLssScanBlock / kWave];
  const int per = (n + kLssScanBlock - 1) / kLssScanBlock;
  const int lo = min((int)threadIdx.x * per, n), hi = min(lo + per, n);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += a[i];
  int total;
  int run = lss_block_excl_scan<kLssScanBlock / kWave>(s, ws, total);
  for (int i = lo; i < hi; ++i) {
    const int t = a[i];
    a[i] = run;
    run += t;
  }
  if (total_out && threadIdx.x == 0) {
    total_out[0] = 0;
    total_out[1] = total;
  }
}

// Digit counts [256][nblocks]: block d scans row d in place (exclusive, over the tiles) and writes the row's sum to
// totals[d]; the scatter adds the exclusive scan of the 256 totals itself.  (One block scanning all 256 x nblocks
// counts took 43 of the prepare's 132 us at BEVDet-R50.)
__global__ __launch_bounds__(kLssBlock) void lss_row_scan_kernel(int *__restrict__ hist, int nblocks,
                                                                 int *__restrict__ totals) {
  __shared__ int ws[kLssWaves];
  int *row = hist + (size_t)blockIdx.x * nblocks;
  int running = 0;
  for (int base = 0; base < nblocks; base += kLssBlock) {
    const int i = base + threadIdx.x;
    const int v = i < nblocks ? row[i] : 0;
    int total;
    const int excl = lss_block_excl_scan<kLssWaves>(v, ws, total);
    if (i < nblocks) row[i] = running + excl;
    running += total;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = running;
}

// One radix pass: element i of the tile goes to offsets[digit][block] + (elements of the tile in front of it with the
// same digit).  FIRST: the payload is the element's own index.
template <bool FIRST>
__global__ __launch_bounds__(kLssBlock) void lss_scatter_kernel(
    const unsigned *__restrict__ keys_in, const int *__restrict__ vals_in, unsigned *__restrict__ keys_out,
    int *__restrict__ vals_out, const int *__restrict__ offsets, const int *__restrict__ totals, int n, int shift,
    int nblocks) {
  __shared__ int base[256];
  __shared__ int cnt[kLssWaves][256];
  __shared__ int ws[kLssWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  int all;
  base[tid] = lss_block_excl_scan<kLssWaves>(totals[tid], ws, all) + offsets[tid * nblocks + blockIdx.x];
#pragma unroll
  for (int w = 0; w < kLssWaves; ++w) cnt[w][tid] = 0;
  __syncthreads();
  for (int j = 0; j < kLssItems; ++j) {
    const int i = blockIdx.x * kLssTile + j * kLssBlock + tid;
    if (blockIdx.x * kLssTile + j * kLssBlock >= n) break;   // uniform
    const bool valid = i < n;
    const unsigned key = valid ? keys_in[i] : 0u;
    const unsigned digit = (key >> shift) & 255u;
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (digit >> b) & 1u;
      const unsigned long long bb = __ballot(bit);
      m &= bit ? bb : ~bb;
    }
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    if (valid && rank == 0) cnt[wave][digit] = __popcll(m);
    __syncthreads();
    if (valid) {
      int pos = base[digit] + rank;
#pragma unroll
      for (int w = 0; w < kLssWaves; ++w)
        if (w < wave) pos += cnt[w][digit];
      if (pos >= 0 && pos < n) {   // always true for consistent counts; never an out-of-bounds store
        keys_out[pos] = key;
        vals_out[pos] = FIRST ? i : vals_in[i];
      }
    }
    __syncthreads();
    int add = 0;
#pragma unroll
    for (int w = 0; w < kLssWaves; ++w) {
      add += cnt[w][tid];
      cnt[w][tid] = 0;
    }
    base[tid] += add;
    __syncthreads();
  }
}

__device__ __forceinline__ bool lss_run_start(const unsigned *__restrict__ sk, int i, unsigned cells) {
  const unsigned k = sk[i];
  return k < cells && (i == 0 || sk[i - 1] != k);
}

// run starts per tile of the sorted keys
__global__ __launch_bounds__(kLssBlock) void lss_flag_count_kernel(const unsigned *__restrict__ sk, int n,
                                                                   unsigned cells, int *__restrict__ block_count) {
  __shared__ int ws[kLssWaves];
  int c = 0;
  for (int j = 0; j < kLssItems; ++j) {
    const int i = blockIdx.x * kLssTile + j * kLssBlock + threadIdx.x;
    if (i < n && lss_run_start(sk, i, cells)) ++c;
  }
  int total;
  lss_block_excl_scan<kLssWaves>(c, ws, total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// the three per-point arrays (zero behind the kept points), the interval starts in order, counts[0]
__global__ __launch_bounds__(kLssBlock) void lss_emit_kernel(
    const unsigned *__restrict__ sk, const int *__restrict__ sv, int n, unsigned cells, int dhw, int hw,
    const int *__restrict__ block_offset, int32_t *__restrict__ ranks_bev, int32_t *__restrict__ ranks_depth,
    int32_t *__restrict__ ranks_feat, int32_t *__restrict__ interval_starts, int cap, int32_t *__restrict__ counts) {
  __shared__ int ws[kLssWaves];
  int running = block_offset[blockIdx.x];
  for (int j = 0; j < kLssItems; ++j) {
    if (blockIdx.x * kLssTile + j * kLssBlock >= n) break;   // uniform
    const int i = blockIdx.x * kLssTile + j * kLssBlock + threadIdx.x;
    bool flag = false;
    if (i < n) {
      const unsigned k = sk[i];
      const bool kept = k < cells;
      const int rd = kept ? sv[i] : 0;
      ranks_bev[i] = kept ? (int)k : 0;
      ranks_depth[i] = rd;
      ranks_feat[i] = (rd / dhw) * hw + rd % hw;
      flag = kept && (i == 0 || sk[i - 1] != k);
      if (kept && (i + 1 == n || sk[i + 1] >= cells)) counts[0] = i + 1;
    }
    int total;
    const int idx = running + lss_block_excl_scan<kLssWaves>(flag ? 1 : 0, ws, total);
    if (flag && idx < cap) interval_starts[idx] = i;
    running += total;
  }
}

__global__ __launch_bounds__(kLssBlock) void lss_lengths_kernel(int32_t *__restrict__ interval_starts,
                                                                int32_t *__restrict__ interval_lengths, int cap,
                                                                const int32_t *__restrict__ counts) {
  const int k = blockIdx.x * kLssBlock + threadIdx.x;
  if (k >= cap) return;
  const int n_pts = counts[0], n_int = counts[1];
  if (k < n_int) {
    interval_lengths[k] = (k + 1 < n_int ? interval_starts[k + 1] : n_pts) - interval_starts[k];
  } else {
    interval_starts[k] = 0;
    interval_lengths[k] = 0;
  }
}

inline size_t lss_round(size_t n) { return (n + 63) & ~(size_t)63; }

inline bool lss_sizes_ok(int n_cams, int d, int h, int w, long &num_points) {
  num_points = (long)n_cams * d * h * w;
  return (long)d * h * w <= kLssMaxPoints && num_points <= kLssMaxPoints;
}

// bytes for num_points points: two (key, payload) buffers, the digit counts [256][nblocks], their 256 row sums, the
// run starts per block
inline size_t lss_workspace_bytes(size_t np) {
  const size_t nblocks = (np + kLssTile - 1) / kLssTile;
  return (4 * lss_round(np) + lss_round(256 * nblocks) + 256 + lss_round(nblocks)) * sizeof(int32_t);
}

// grid_host -> g (nx, nxy, cells excepted); BEVOPS_BAD_PARAM for a value no grid can hold
inline int lss_read_grid(const float *grid_host, LssGrid &g) {
  for (int a = 0; a < 3; ++a) {
    g.lower[a] = grid_host[a];
    g.interval[a] = grid_host[3 + a];
    g.size[a] = grid_host[6 + a];
    if (!isfinite(g.lower[a]) || !isfinite(g.interval[a]) || !(g.interval[a] > 0.f)) return BEVOPS_BAD_PARAM;
    if (!isfinite(g.size[a]) || !(g.size[a] >= 1.f)) return BEVOPS_BAD_PARAM;
  }
  return BEVOPS_SUCCESS;
}

// cells = nx ny nz, or -1 when a size is not integral or the product exceeds kLssMaxCells
inline double lss_cells(const LssGrid &g) {
  double cells = 1.0;
  for (int a = 0; a < 3; ++a) {
    if (g.size[a] != floorf(g.size[a]) || g.size[a] > (float)kLssMaxCells) return -1.0;
    cells *= (double)g.size[a];
  }
  return cells > (double)kLssMaxCells ? -1.0 : cells;
}

// The launches of both entries; every limit has been checked: n = batch * n_cams * d * h * w <= kLssMaxPoints,
// batch * g.cells <= kLssMaxCells, the workspace holds lss_workspace_bytes(n).
int lss_launch(const float *frustum, const float *calib, const LssGrid &g, int32_t *ranks_bev, int32_t *ranks_depth,
               int32_t *ranks_feat, int32_t *interval_starts, int32_t *interval_lengths, int32_t *counts, float *coor,
               int batch, int n_cams, int d, int h, int w, void *workspace, hipStream_t st) {
  const int dhw = d * h * w, hw = h * w, n = batch * n_cams * dhw;
  const int calib_stride = n_cams * 24 + 9;
  const unsigned all_cells = (unsigned)batch * (unsigned)g.cells;
  const int nblocks = (n + kLssTile - 1) / kLssTile;
  const int cap = (unsigned)n < all_cells ? n : (int)all_cells;
  int32_t *ws = static_cast<int32_t *>(workspace);
  unsigned *keys[2] = {(unsigned *)ws, (unsigned *)(ws + 2 * lss_round(n))};
  int *vals[2] = {ws + lss_round(n), ws + 3 * lss_round(n)};
  int *hist = ws + 4 * lss_round(n);
  int *totals = hist + lss_round((size_t)256 * nblocks);
  int *block_count = totals + 256;

  int passes = 1;   // digits that hold the value `all_cells` (the key of a dropped point)
  while (passes < 4 && (all_cells >> (8 * passes)) != 0) ++passes;

  hipLaunchKernelGGL(lss_cell_kernel, dim3(nblocks), dim3(kLssBlock), 0, st, frustum, calib, g, n_cams, calib_stride,
                     all_cells, dhw, n, keys[0], hist, nblocks, coor);
  int src = 0;
  for (int p = 0; p < passes; ++p) {
    if (p > 0)
      hipLaunchKernelGGL(lss_hist_kernel, dim3(nblocks), dim3(kLssBlock), 0, st, keys[src], n, 8 * p, hist, nblocks);
    hipLaunchKernelGGL(lss_row_scan_kernel, dim3(256), dim3(kLssBlock), 0, st, hist, nblocks, totals);
    if (p == 0)
      hipLaunchKernelGGL(lss_scatter_kernel<true>, dim3(nblocks), dim3(kLssBlock), 0, st, keys[src], vals[src],
                         keys[src ^ 1], vals[src ^ 1], hist, totals, n, 0, nblocks);
    else
      hipLaunchKernelGGL(lss_scatter_kernel<false>, dim3(nblocks), dim3(kLssBlock), 0, st, keys[src], vals[src],
                         keys[src ^ 1], vals[src ^ 1], hist, totals, n, 8 * p, nblocks);
    src ^= 1;
  }
  hipLaunchKernelGGL(lss_flag_count_kernel, dim3(nblocks), dim3(kLssBlock), 0, st, keys[src], n, all_cells,
                     block_count);
  hipLaunchKernelGGL(lss_scan_kernel, dim3(1), dim3(kLssScanBlock), 0, st, block_count, nblocks, counts);
  hipLaunchKernelGGL(lss_emit_kernel, dim3(nblocks), dim3(kLssBlock), 0, st, keys[src], vals[src], n, all_cells, dhw,
                     hw, block_count, ranks_bev, ranks_depth, ranks_feat, interval_starts, cap, counts);
  hipLaunchKernelGGL(lss_lengths_kernel, dim3((cap + kLssBlock - 1) / kLssBlock), dim3(kLssBlock), 0, st,
                     interval_starts, interval_lengths, cap, counts);
  return launch_status();
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" size_t bevops_lss_voxel_prepare_workspace_size(int n_cams, int d, int h, int w) {
  if (n_cams <= 0 || d <= 0 || h <= 0 || w <= 0) return 0;
  if ((long)n_cams * d > kLssMaxPoints || (long)h * w > kLssMaxPoints) return 0;
  long np;
  if (!lss_sizes_ok(n_cams, d, h, w, np)) return 0;
  return lss_workspace_bytes((size_t)np);
}

extern "C" int bevops_lss_voxel_prepare(const float *frustum, const float *calib, const float *grid_host,
                                        int32_t *ranks_bev, int32_t *ranks_depth, int32_t *ranks_feat,
                                        int32_t *interval_starts, int32_t *interval_lengths, int32_t *counts,
                                        float *coor, int batch, int n_cams, int d, int h, int w, void *workspace,
                                        size_t workspace_bytes, void *stream) {
  if (!frustum || !calib || !grid_host || !ranks_bev || !ranks_depth || !ranks_feat || !interval_starts ||
      !interval_lengths || !counts || !workspace)
    return BEVOPS_BAD_PARAM;
  if (batch <= 0 || n_cams <= 0 || d <= 0 || h <= 0 || w <= 0) return BEVOPS_BAD_PARAM;
  LssGrid g;
  if (lss_read_grid(grid_host, g) != BEVOPS_SUCCESS) return BEVOPS_BAD_PARAM;
  if (batch != 1) return BEVOPS_NOT_SUPPORTED;
  if ((long)n_cams * d > kLssMaxPoints || (long)h * w > kLssMaxPoints) return BEVOPS_NOT_SUPPORTED;
  long np;
  if (!lss_sizes_ok(n_cams, d, h, w, np)) return BEVOPS_NOT_SUPPORTED;
  const double cells = lss_cells(g);
  if (cells < 0.0) return BEVOPS_NOT_SUPPORTED;
  if (workspace_bytes < bevops_lss_voxel_prepare_workspace_size(n_cams, d, h, w) || !aligned16(workspace))
    return BEVOPS_BAD_PARAM;
  g.nx = (int)g.size[0];
  g.nxy = g.nx * (int)g.size[1];
  g.cells = (int)cells;
  return lss_launch(frustum, calib, g, ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths, counts,
                    coor, 1, n_cams, d, h, w, workspace, static_cast<hipStream_t>(stream));
}

namespace {
// num_points over the batch, or -1 beyond kLssMaxPoints (every partial product is tested, so nothing overflows)
long lss_batched_points(int batch, int n_cams, int d, int h, int w) {
  long np = 1;
  const int f[5] = {batch, n_cams, d, h, w};
  for (int v : f) {
    np *= v;
    if (np > kLssMaxPoints) return -1;
  }
  return np;
}
}  // namespace

extern "C" size_t bevops_lss_voxel_prepare_batched_workspace_size(int batch, int n_cams, int d, int h, int w) {
  if (batch <= 0 || n_cams <= 0 || d <= 0 || h <= 0 || w <= 0) return 0;
  const long np = lss_batched_points(batch, n_cams, d, h, w);
  return np < 0 ? 0 : lss_workspace_bytes((size_t)np);
}

extern "C" int bevops_lss_voxel_prepare_batched(const float *frustum, const float *calib, const float *grid_host,
                                                int32_t *ranks_bev, int32_t *ranks_depth, int32_t *ranks_feat,
                                                int32_t *interval_starts, int32_t *interval_lengths, int32_t *counts,
                                                float *coor, int batch, int n_cams, int d, int h, int w,
                                                void *workspace, size_t workspace_bytes, void *stream) {
  if (!frustum || !calib || !grid_host || !ranks_bev || !ranks_depth || !ranks_feat || !interval_starts ||
      !interval_lengths || !counts || !workspace)
    return BEVOPS_BAD_PARAM;
  if (batch <= 0 || n_cams <= 0 || d <= 0 || h <= 0 || w <= 0) return BEVOPS_BAD_PARAM;
  LssGrid g;
  if (lss_read_grid(grid_host, g) != BEVOPS_SUCCESS) return BEVOPS_BAD_PARAM;
  if (lss_batched_points(batch, n_cams, d, h, w) < 0) return BEVOPS_NOT_SUPPORTED;
  const double cells = lss_cells(g);
  if (cells < 0.0 || cells * (double)batch > (double)kLssMaxCells) return BEVOPS_NOT_SUPPORTED;
  if (workspace_bytes < bevops_lss_voxel_prepare_batched_workspace_size(batch, n_cams, d, h, w) ||
      !aligned16(workspace))
    return BEVOPS_BAD_PARAM;
  g.nx = (int)g.size[0];
  g.nxy = g.nx * (int)g.size[1];
  g.cells = (int)cells;
  return lss_launch(frustum, calib, g, ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths, counts,
                    coor, batch, n_cams, d, h, w, workspace, static_cast<hipStream_t>(stream));
}
