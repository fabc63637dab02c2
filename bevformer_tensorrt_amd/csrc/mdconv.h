// Shared pieces of the DCNv2 translation units (mdconv.hip: fp32 / fp16; mdconv_s8.hip: int8).
#ifndef BEVOPS_MDCONV_H_
#define BEVOPS_MDCONV_H_
#include <type_traits>

#include "common.h"

namespace bevops {
// The three ways a call can run, and what bevops_mdconv_set_variant can force per dtype family
enum DcnPath {
  kDcnAuto = 0,   // (variant only) the plan decides
  kDcnLds,        // LDS-DMA pipelined implicit GEMM (sections 5c, 6c)
  kDcnStaged,     // register-staged fused implicit GEMM (sections 5, 6b)
  kDcnGemm        // im2col + GEMM (sections 3, 4, 6)
};

// bevops_mdconv_set_variant, decoded once (kDcnVariants in mdconv.hip is the only place that knows the numbers).
// A value acts on BOTH dtype families:
//   0      automatic
//   1 2 3  fp16: im2col + GEMM / register-staged kernel with 256 / with 512 threads;       int8: automatic
//   4      both: no split-K tail (fp16 also keeps the 64-pixel tiles);   5  both: 128-pixel tiles whatever the tile count
//   6 8 9  int8: im2col + GEMM / register-staged kernel / LDS-DMA kernel whatever the tile count;
//          fp16: a call inside the fused domain runs on the 512-thread register-staged kernel, as under 3
//   10 14 15  as 0 / 4 / 5, the fp16 LDS-DMA kernel with the skeleton it had before the footprint table: every thread
//          computes its pixel's sampling footprint per tap, channels-last outputs leave by 8-byte stores per lane.  The
//          A/B partner of the default: the same bits, in one process (tests/test_mdconv_skeleton_gpu.py, tools/dcn_time.py)
//   20 24 25  as 0 / 4 / 5 with the footprint table but the per-lane stores (the table's share of the gain alone)
// Any other value selects the automatic choice, exactly as 0 does (the rule of bevops_msda_set_variant).
enum DcnSkeleton {
  kDcnSkelFull = 0,   // footprint table in LDS (128-pixel tiles, <= kDcnTabTaps taps) + row-wide channels-last stores
  kDcnSkelParent,     // per-thread footprints, per-lane stores
  kDcnSkelTable       // footprint table, per-lane stores
};
struct DcnVariant {
  int id;            // what bevops_mdconv_set_variant returns as the previous value
  DcnPath f16, s8;   // forced path of the family, kDcnAuto = none
  int f16_threads;   // block size of the fp16 register-staged kernel when f16 == kDcnStaged
  bool no_tail, wide;
  DcnSkeleton skel;  // fp16 LDS-DMA kernel only
};
extern thread_local DcnVariant g_dcn_variant;   // defined in mdconv.hip

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvDims {
  int B, Cin, H, W, Cout, Kh, Kw, sh, sw, ph, pw, dh, dw, G, DG, Ho, Wo;
};

template <typename T> __device__ __forceinline__ float tof(T v);
template <> __device__ __forceinline__ float tof<float>(float v) { return v; }
template <> __device__ __forceinline__ float tof<__half>(__half v) { return __half2float(v); }
template <typename T> __device__ __forceinline__ T fromf(float v);
template <> __device__ __forceinline__ float fromf<float>(float v) { return v; }
template <> __device__ __forceinline__ __half fromf<__half>(float v) { return __float2half_rn(v); }

// ---- 1. NCHW -> NHWC ------------------------------------------------------------
// `flip` (int8 only): XOR applied to every byte -- 0x80 makes the copy hold v + 128 as u8 (the
// fused int8 kernel's operand form, dcn_fused_s8_kernel)
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const T *__restrict__ in,
                                                           T *__restrict__ out, int C, int HW, int flip = 0) {
  __shared__ T tile[32][33];
  const int b = blockIdx.z;
  const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const T *ib = in + (size_t)b * C * HW;
  T *ob = out + (size_t)b * C * HW;
#pragma unroll
  for (int r = 0; r < 32; r += 8) {
    const int c = c0 + ty + r, p = p0 + tx;
    if (c < C && p < HW) {
      if constexpr (sizeof(T) == 1) tile[ty + r][tx] = (T)(ib[(size_t)c * HW + p] ^ (T)flip);
      else tile[ty + r][tx] = ib[(size_t)c * HW + p];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 32; r += 8) {
    const int p = p0 + ty + r, c = c0 + tx;
    if (c < C && p < HW) ob[(size_t)p * C + c] = tile[tx][ty + r];
  }
}

// ---- 2. weight [Cout][Cin/g][KK] -> [Cout][KK][Cin/g] ------------------------------
template <typename T>
__global__ __launch_bounds__(256) void repack_weight_kernel(const T *__restrict__ w,
                                                            T *__restrict__ wt, int Cout,
                                                            int cin_g, int KK, int row_stride) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)Cout * cin_g * KK;
  if (i >= total) return;
  const int ci = (int)(i % cin_g);
  const int t = (int)((i / cin_g) % KK);
  const size_t co = i / ((size_t)cin_g * KK);
  wt[co * row_stride + (size_t)t * cin_g + ci] = w[(co * cin_g + ci) * KK + t];
}

// fp16 / int8 GEMM tile (sections 4a, 6) and its scatter epilogue
constexpr int kBM = 128, kBN = 128, kBK = 32, kLd = kBK + 8;  // +8 halves: conflict-free b128 reads

struct GemmEpi {
  int HoWo, Cout, co0;  // out[(n / HoWo) * Cout + co0 + m][n % HoWo]
};

// fused implicit-GEMM block tile (section 5)
constexpr int kFM = 256, kFN = 64, kFK = 64, kFLd = kFK + 8;

// LDS image of the LDS-DMA kernels (sections 5c, 6c)
constexpr int kGA = kFM * kFK * 2;  // 32 KB weight tile image
// WN = wave columns (each 32 pixels): 2 -> 512 threads, 64-pixel tile, 80 KB LDS, 2 blocks per CU;
//                                      4 -> 1024 threads, 128-pixel tile, 96 KB LDS, 1 block per CU
//                                           (the weight tile is fetched once per 128 pixels; fp16: + 4 KB per tap of
//                                           footprint table behind it, kDcnTabTap)
template <int WN> struct Glds {
  static constexpr int kN = 32 * WN;          // pixels per tile
  static constexpr int kThreads = 256 * WN;
  static constexpr int kB = kN * kFK * 2;     // pixel tile image bytes
  static constexpr int kLds = 2 * (kGA + kB);
  static constexpr int kPieces = 32 / (4 * WN);  // 1 KB weight DMA pieces per wave
};

// Footprint table of the fp16 LDS-DMA kernel (128-pixel tiles only: two 64-pixel blocks already fill the CU's 160 KB):
// per tap 128 records of 4 corner byte offsets, then 128 records of 4 packed blend weights, behind the A/B buffers.
constexpr int kDcnTabTap = 2 * Glds<4>::kN * 16;                 // bytes per tap
constexpr int kDcnTabTaps = (160 * 1024 - Glds<4>::kLds) / kDcnTabTap;   // 16: a 5 x 5 kernel keeps the per-thread footprint
// channels-last epilogue image [pixel][kFM halves]: rows padded by 16 bytes (b128 row reads stay aligned and
// conflict-free, the 8-byte accumulator writes are 2-way conflicted instead of 16-way)
constexpr int kDcnEpiRow = kFM * 2 + 16;
static_assert(Glds<4>::kN * kDcnEpiRow <= Glds<4>::kLds && Glds<2>::kN * kDcnEpiRow <= Glds<2>::kLds, "epilogue image");

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ unsigned swz8(unsigned r) { return (r ^ (r >> 3)) & 7u; }

// Tail handling: when the tile count leaves a sparsely filled last round (base stage 3: 544 tiles
// on 512 resident blocks -- a round costs the same ~36 dependent k-steps however few blocks run),
// the leftover `tail_tiles` tiles are split `split` ways along K (whole taps) into short blocks
// that come FIRST in the grid; each writes its fp32 partial accumulators to the workspace and
// dcn_tail_finish_kernel adds them in a fixed order (deterministic, no atomics).
struct TailPlan {
  int tail_tiles, split, main_tiles;  // grid.x = tail_tiles * split + main_tiles
  float *partial;                     // [split][tail_tiles][Cout tiles][8 quads][threads] float4
  int out_nhwc, relu;                 // epilogue: output layout [B,Ho,Wo,Cout], fused ReLU
  int om_channels;                    // > 0: `offset` is the raw [B,Ho,Wo,om_channels] output of the pack's
                                      // offset convolution (2*KK offsets, then KK mask logits): sigmoid here
  int row_store;                      // fp16 channels-last: main blocks stage the tile in LDS and store whole pixel rows
};

// ---- host side: problem description and workspace layout -------------------------------------------
inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

inline bool make_dims(ConvDims &d, int B, int Cin, int H, int W, int Cout, int Kh, int Kw, int sh, int sw,
               int ph, int pw, int dh, int dw, int G, int DG) {
  if (B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Kh <= 0 || Kw <= 0 || sh <= 0 ||
      sw <= 0 || ph < 0 || pw < 0 || dh <= 0 || dw <= 0 || G <= 0 || DG <= 0)
    return false;
  if (Cin % G || Cout % G || Cin % DG) return false;
  const int Ho = (H + 2 * ph - (dh * (Kh - 1) + 1)) / sh + 1;
  const int Wo = (W + 2 * pw - (dw * (Kw - 1) + 1)) / sw + 1;
  if (Ho <= 0 || Wo <= 0) return false;
  d = ConvDims{B, Cin, H, W, Cout, Kh, Kw, sh, sw, ph, pw, dh, dw, G, DG, Ho, Wo};
  return true;
}

struct WsLayout {
  size_t xt, wt, col, total;
};
// int8 GEMM rows are padded to a multiple of 16 bytes (zero filled)
inline size_t kpad(const ConvDims &d, size_t es) {
  const size_t kg = (size_t)(d.Cin / d.G) * d.Kh * d.Kw;
  return es == 1 ? ((kg + 15) & ~size_t(15)) : kg;
}
inline WsLayout ws_layout(const ConvDims &d, size_t es) {
  WsLayout w;
  const size_t kp = kpad(d, es);
  w.xt = 0;
  w.wt = align256((size_t)d.B * d.Cin * d.H * d.W * es);
  w.col = w.wt + align256((size_t)d.Cout * kp * es);
  w.total = w.col + align256((size_t)d.B * d.Ho * d.Wo * d.G * kp * es);
  return w;
}

// ---- host side: one call descriptor, one plan ------------------------------------------------------
// Everything a forward call carries.  Every extern "C" entry fills one, validates it and hands it to its family's
// plan_* / launch_* pair (mdconv.hip: fp32 / fp16, mdconv_s8.hip: int8).
struct DcnCall {
  ConvDims d;        // d.B == 0: make_dims rejected the 15 geometry ints
  int dtype;         // BEVOPS_F32 / BEVOPS_F16 / BEVOPS_I8
  const void *input, *offset, *mask, *weight, *bias;
  void *output;
  bool packed;       // `weight` is the image made by bevops_mdconv_pack_weight
  bool nhwc;         // channels-last input and output (int8: the engine's block, raw fp16 offsets / mask logits)
  bool relu;
  bool exact;        // int8 nhwc: the plugin's two requantisations per column element, not the folded one
  int om_channels;   // > 0: `offset` is the raw [B, Ho, Wo, om_channels] output of the pack's offset convolution
  float s_in, s_off, s_mask, s_w, s_out;   // int8: per-tensor scales
  void *workspace;
  size_t workspace_bytes;
  hipStream_t stream;
};

inline DcnCall dcn_call(int dtype, const void *input, const void *offset, const void *mask, const void *weight,
                        const void *bias, void *output, void *workspace, size_t workspace_bytes, int B, int Cin, int H,
                        int W, int Cout, int Kh, int Kw, int sh, int sw, int ph, int pw, int dh, int dw, int G, int DG,
                        void *stream) {
  DcnCall c{};
  (void)make_dims(c.d, B, Cin, H, W, Cout, Kh, Kw, sh, sw, ph, pw, dh, dw, G, DG);
  c.dtype = dtype;
  c.input = input, c.offset = offset, c.mask = mask, c.weight = weight, c.bias = bias, c.output = output;
  c.workspace = workspace, c.workspace_bytes = workspace_bytes;
  c.stream = static_cast<hipStream_t>(stream);
  return c;
}

// split-K tail of the LDS-DMA kernels (see TailPlan): `left` tiles of a sparsely filled last round, `split` ways
struct DcnTail {
  int tiles, split;
};
// blocks = grid.x * grid_y of the untailed launch, slots = resident blocks of the device, room = bytes the workspace
// can give to the partial sums, block_bytes = what one block parks there (its threads' 32 accumulators)
inline DcnTail plan_tail(int blocks, int grid_y, int KK, int slots, size_t room, size_t block_bytes) {
  if (blocks <= slots || grid_y != 1) return DcnTail{0, 1};
  const int left = blocks % slots;
  int split = 0;
  for (int f = KK; f >= 2; --f)
    if (KK % f == 0 && left * f <= slots) { split = f; break; }
  if (left > 0 && left * 2 <= slots && split >= 2 && room >= (size_t)split * left * block_bytes) return DcnTail{left, split};
  return DcnTail{0, 1};
}

// What a call will launch.  Made by plan_fp / plan_s8 before anything is queued; a rejected call queues nothing.
enum DcnCopy { kDcnCopyNone, kDcnCopyGeneric, kDcnCopyQuad };   // NCHW -> NHWC: none (nhwc), 32 x 32 tiles, 4 x 4 register transposes
struct DcnPlan {
  DcnPath path;     // kDcnLds: every conv group that reads ONE deform group runs the LDS-DMA kernel, any other group
                    // the register-staged one (int8: kDcnLds only when all groups do)
  int threads;      // fp16 register-staged kernel: 256 or 512
  int WN;           // LDS-DMA kernel: wave columns, 2 (64-pixel tiles) or 4 (128-pixel tiles)
  DcnTail tail;
  char *partial;    // LDS-DMA kernel: where the tail's partial sums go
  DcnCopy copy;
  bool repack;      // weights re-laid out per call (not packed by the caller)
  bool zero_pad;    // int8, ragged K: packed weights and columns zeroed first
  bool table;       // fp16 LDS-DMA kernel: sampling footprints from the block's LDS table (else per thread)
  bool row_store;   // fp16 LDS-DMA kernel, channels-last: row-wide stores through LDS (else per lane)
};
// the device's CU count, <= 0 when HIP cannot tell; the resident blocks of the LDS-DMA kernel of tile width wn
typedef int (*DcnCusFn)();
typedef int (*DcnSlotsFn)(const DcnCall &c, int wn);

// conv group g reads ONE deform group (the LDS-DMA kernels' domain: dg constant over a block's k-loop)
inline bool one_deform_group(const ConvDims &d, int g) {
  const int cin_g = d.Cin / d.G, cin_dg = d.Cin / d.DG;
  return cin_g <= cin_dg && (g * cin_g) / cin_dg == (g * cin_g + cin_g - 1) / cin_dg;
}
inline bool one_deform_group(const ConvDims &d) {
  for (int g = 0; g < d.G; ++g)
    if (!one_deform_group(d, g)) return false;
  return true;
}

inline int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  return cus;
}

// blocks of Kern (threads, dynamic LDS bytes) the device holds at once, 0 on failure; sets the kernel's dynamic LDS
// limit on the way.  Cached per thread, kernel and device.
template <auto Kern>
int resident_blocks(int threads, int lds) {
  static thread_local int cached_dev = -1, cached = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (dev == cached_dev) return cached;
  int per_cu = 0;
  const int cus = device_cus();
  if (cus <= 0 ||
      hipFuncSetAttribute(reinterpret_cast<const void *>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kern, threads, lds) != hipSuccess)
    return 0;
  cached_dev = dev;
  cached = per_cu * cus;
  return cached;
}

}  // namespace
}  // namespace bevops
#endif  // BEVOPS_MDCONV_H_
