// FlashOcc's occupancy predictor behind final_conv in ONE launch (bevops_occ_head_f16; BEVOCCHead2D's
// Linear(C, Hd) + Softplus + Linear(Hd, Dz Ncls) + argmax over the classes; bevformer_tensorrt_amd/bevdet.py,
// design/flashocc.md):
//     h[m, j]     = fp16( softplus( b1[j] + sum_c y[m, c] W1[j, c] ) )            fp32 sum, fp32 Softplus, ONE rounding
//     logit[m, n] = b2[n] + sum_j h[m, j] W2[n, j]                                fp32, n = z Ncls + cls
//     occ[m, z]   = the lowest cls whose logit[m, z Ncls + cls] is the largest of voxel z, on the fp32 values
// Neither h nor the logits reach memory (the logits only when the caller asks for them).
//
// MI355X mapping.  A block of 256 threads owns 128 rows, a wave 32 of them and ALL columns, so nothing about a row ever
// crosses a wave.  ONE wave per SIMD (__launch_bounds__(256, 1), up to 512 registers a lane) because the launch keeps
// three things in registers for the whole block:
//   * the wave's y rows as the B fragments of v_mfma_f32_32x32x16_f16 (C / 16 fragments of 16 bytes: 64 VGPRs at C = 256),
//     loaded once;
//   * the second GEMM's 32 x (32 kNB) fp32 accumulators (176 registers);
//   * the first GEMM's 32 x 64 accumulators of the current slab of hidden columns (32 registers).
// The hidden tensor is produced 64 columns at a time and NEVER LEAVES THE REGISTERS: with the weight rows as operand A a
// lane's accumulator holds 16 hidden values of ONE row m = lane & 31 (columns 32 i + 8 g + 4 (lane >> 5) + c), and the B
// fragment of the next GEMM wants 8 k-values of that same row.  Which k-values is only a naming: pack_occ_head orders
// W2's k inside a slab so that the lane's own values, rounded once and packed, ARE its fragment (position 8 hb + 4 q + c
// of k-step (i, p) is hidden column 32 i + 16 p + 8 q + 4 hb + c).  No LDS slab, no barrier between the two GEMMs.
// LDS holds the weights only, whatever Hd is: the slab's 64 rows of W1 and the slab's k-slice of W2, 84 480 bytes.  They
// are register-staged one phase ahead: W2's slice is requested from memory before the first GEMM of the slab and stored
// behind it, the next slab's W1 is requested before the second GEMM and stored behind it: two barriers a slab.
// Epilogue without LDS: pack_occ_head also orders W2's ROWS: the lane half hb = lane >> 5 receives the voxels z with
// z & 1 == hb, class-contiguous, in the order it walks its accumulators; a running maximum with a strict > keeps the
// lowest class.  Rows of W2 that padding added belong to no voxel and are never compared.  The two halves exchange their
// 8 bytes through one cross-lane read and the row leaves as one 16-byte store when Dz = 16.
#include "tile_mma.h"

namespace bevops {
namespace {

constexpr int kOccRows = 128;                  // rows per block
constexpr int kOccNB = 11;                     // 32-column blocks of the second GEMM a wave can hold
constexpr int kOccKS = 16;                     // 16-channel steps of the first GEMM (C <= 256)
constexpr int kOccW2Ld = 128 + 16;             // LDS row of the W2 slice: 64 k-values + pad
constexpr int kOccW1Bytes = 64 * (2 * 256 + 16);
constexpr int kOccLds = kOccW1Bytes + kOccNB * 32 * kOccW2Ld;

struct OccArgs {
  const __half *y, *w1, *b1, *w2, *b2;
  unsigned char *occ;
  __half *logits;
  long long rows, s_img, s_line, s_px;          // output bytes per image / line / pixel
  int y_pitch, C, Hd, Dz, Ncls, nb, H, W, vec16;
};

// torch's Softplus (beta 1, threshold 20) on the hardware exp2 / log2: v itself above 20, else ln2 log2(1 + exp2(v log2e))
__device__ __forceinline__ float softplus_f32(float v) {
  const float t = __builtin_amdgcn_exp2f(v * 1.44269504088896340736f);
  const float s = 0.69314718055994530942f * __builtin_amdgcn_logf(1.f + t);
  return v > 20.f ? v : s;
}

__global__ __launch_bounds__(256, 1) void occ_head_kernel(OccArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *W1s = smem, *W2s = smem + kOccW1Bytes;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hb = lane >> 5;
  const int C = p.C, nb = p.nb, nslab = p.Hd / 64;
  const int w1ld = 2 * C + 16;                 // LDS row of the W1 slab (an odd number of 16-byte units: conflict-free)
  const long long m = (long long)blockIdx.x * kOccRows + wave * 32 + l31;
  const bool row_ok = m < p.rows;

  // the wave's y rows, resident: fragment ks = channels 16 ks + 8 hb .. + 7 of row m (zeros past the last row)
  i32x4_t yf[kOccKS];
#pragma unroll
  for (int ks = 0; ks < kOccKS; ++ks) {
    yf[ks] = i32x4_t{0, 0, 0, 0};
    if (ks * 16 < C && row_ok) yf[ks] = *reinterpret_cast<const i32x4_t *>(p.y + m * p.y_pitch + ks * 16 + hb * 8);
  }
  f32x16_t acc2[kOccNB];
#pragma unroll
  for (int j = 0; j < kOccNB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[j][r] = 0.f;

  // staging: W1's slab is 64 C / 8 chunks of 16 bytes (C / 32 a thread), W2's slice 256 nb chunks (nb a thread); both are
  // contiguous in memory and chunk q of a thread is tid + 256 j
  i32x4_t st[kOccNB];
  const i32x4_t *w1g = reinterpret_cast<const i32x4_t *>(p.w1), *w2g = reinterpret_cast<const i32x4_t *>(p.w2);
  const int cpr = C / 8;                       // chunks per W1 row
  auto w1_load = [&](int s) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j * 32 < C) st[j] = w1g[(size_t)s * 64 * cpr + tid + 256 * j];
  };
  auto w1_store = [&]() {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j * 32 < C) {
        const int q = tid + 256 * j;
        *reinterpret_cast<i32x4_t *>(W1s + (q / cpr) * w1ld + (q % cpr) * 16) = st[j];
      }
  };
  auto w2_load = [&](int s) {
#pragma unroll
    for (int j = 0; j < kOccNB; ++j)
      if (j < nb) st[j] = w2g[(size_t)s * 256 * nb + tid + 256 * j];
  };
  auto w2_store = [&]() {
#pragma unroll
    for (int j = 0; j < kOccNB; ++j)
      if (j < nb) *reinterpret_cast<i32x4_t *>(W2s + ((tid >> 3) + 32 * j) * kOccW2Ld + (tid & 7) * 16) = st[j];
  };

  w1_load(0);
  w1_store();
  __syncthreads();
  for (int s = 0; s < nslab; ++s) {
    w2_load(s);
    // ---- first GEMM: the slab's 64 hidden columns of the wave's 32 rows
    f32x16_t acc1[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[i][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < kOccKS; ++ks)
      if (ks * 16 < C) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const i32x4_t a = *reinterpret_cast<const i32x4_t *>(W1s + (i * 32 + l31) * w1ld + ks * 32 + hb * 16);
          acc1[i] = mma(a, yf[ks], acc1[i]);
        }
      }
    // ---- bias, Softplus in fp32, ONE rounding: the lane's own 32 values as its four B fragments
    i32x4_t hf[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint2 bq = *reinterpret_cast<const uint2 *>(p.b1 + s * 64 + i * 32 + g * 8 + hb * 4);
        const float h0 = softplus_f32(acc1[i][4 * g + 0] + h2f_lo(bq.x)), h1 = softplus_f32(acc1[i][4 * g + 1] + h2f_hi(bq.x));
        const float h2 = softplus_f32(acc1[i][4 * g + 2] + h2f_lo(bq.y)), h3 = softplus_f32(acc1[i][4 * g + 3] + h2f_hi(bq.y));
        hf[i][g >> 1][2 * (g & 1)] = (int)pack_h2(h0, h1);
        hf[i][g >> 1][2 * (g & 1) + 1] = (int)pack_h2(h2, h3);
      }
    w2_store();                                // (every wave left the last slab's second GEMM through its closing barrier)
    if (s + 1 < nslab) w1_load(s + 1);
    __syncthreads();                           // W2's slice is visible; every wave has left this slab's first GEMM
    // ---- second GEMM: the slab as four k-steps of 16
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int j = 0; j < kOccNB; ++j)
        if (j < nb) {
          const i32x4_t a = *reinterpret_cast<const i32x4_t *>(W2s + (j * 32 + l31) * kOccW2Ld + kk * 32 + hb * 16);
          acc2[j] = mma(a, hf[kk >> 1][kk & 1], acc2[j]);
        }
    if (s + 1 < nslab) w1_store();             // (the first GEMM's reads of W1s ended in front of the barrier above)
    __syncthreads();
  }

  // ---- epilogue: b2 in fp32, the running argmax of this lane half's voxels (z = 2 zl + hb), optional fp16 logits
  const int Ncls = p.Ncls, nzl = (p.Dz - hb + 1) >> 1;
  __half *lrow = (p.logits && row_ok) ? p.logits + m * ((long long)p.Dz * Ncls) + hb * Ncls : nullptr;
  unsigned long long mine = 0ull;
  float best = 0.f;
  int bi = 0, cnt = 0, zl = 0;
#pragma unroll
  for (int j = 0; j < kOccNB; ++j)
    if (j < nb) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint2 bq = *reinterpret_cast<const uint2 *>(p.b2 + j * 32 + g * 8 + hb * 4);
        const float bs[4] = {h2f_lo(bq.x), h2f_hi(bq.x), h2f_lo(bq.y), h2f_hi(bq.y)};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float v = acc2[j][4 * g + c] + bs[c];
          if (lrow && zl < nzl) lrow[(long long)zl * 2 * Ncls + cnt] = __float2half(v);
          const bool take = cnt == 0 || v > best;          // strict: a tie keeps the lower class
          best = take ? v : best;
          bi = take ? cnt : bi;
          if (++cnt == Ncls) {
            if (zl < nzl) mine |= (unsigned long long)bi << (8 * zl);
            ++zl;
            cnt = 0;
          }
        }
      }
    }
  // the other half's bytes: lane ^ 32 holds the same row
  const unsigned olo = (unsigned)__shfl((int)(unsigned)mine, lane ^ 32, 64);
  const unsigned ohi = (unsigned)__shfl((int)(unsigned)(mine >> 32), lane ^ 32, 64);
  if (hb != 0 || !row_ok) return;
  const unsigned long long odd = ((unsigned long long)ohi << 32) | olo;
  unsigned wd[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {                // byte z of the row: voxel z, even z from this lane, odd z from the other
    const unsigned e0 = (unsigned)(mine >> (16 * w)) & 0xffu, e1 = (unsigned)(mine >> (16 * w + 8)) & 0xffu;
    const unsigned o0 = (unsigned)(odd >> (16 * w)) & 0xffu, o1 = (unsigned)(odd >> (16 * w + 8)) & 0xffu;
    wd[w] = e0 | (o0 << 8) | (e1 << 16) | (o1 << 24);
  }
  const long long per = (long long)p.H * p.W, b = m / per, pix = m - b * per, yy = pix / p.W, xx = pix - yy * p.W;
  unsigned char *dst = p.occ + b * p.s_img + yy * p.s_line + xx * p.s_px;
  if (p.vec16) {
    *reinterpret_cast<uint4 *>(dst) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
  } else {
#pragma unroll
    for (int z = 0; z < 16; ++z)
      if (z < p.Dz) dst[z] = (unsigned char)(wd[z >> 2] >> (8 * (z & 3)));
  }
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_occ_head_blocks(int Dz, int Ncls) {
  if (Dz < 1 || Ncls < 1 || Dz > 16 || Ncls > 32 || Dz * Ncls > 320) return 0;
  return (((Dz + 1) / 2) * Ncls + 15) / 16;
}

extern "C" int bevops_occ_head_f16(const void *y, int y_pitch, const void *w1, const void *b1, const void *w2_packed,
                                   const void *b2_packed, void *occ, long long occ_stride_image, long long occ_stride_line,
                                   long long occ_stride_pixel, void *logits, int B, int H, int W, int C, int Hd, int Dz,
                                   int Ncls, void *stream) {
  if (!y || !w1 || !b1 || !w2_packed || !b2_packed || !occ) return BEVOPS_BAD_PARAM;
  if (B < 0 || H <= 0 || W <= 0 || C <= 0 || Hd <= 0 || Dz <= 0 || Ncls <= 0) return BEVOPS_BAD_PARAM;
  if (y_pitch < C || y_pitch % 8 != 0) return BEVOPS_BAD_PARAM;
  if (occ_stride_pixel < Dz || occ_stride_line < 0 || occ_stride_image < 0) return BEVOPS_BAD_PARAM;
  if (misaligned(y, 15u) || misaligned(w1, 15u) || misaligned(b1, 15u) || misaligned(w2_packed, 15u) ||
      misaligned(b2_packed, 15u) || (logits && misaligned(logits, 1u)))
    return BEVOPS_BAD_PARAM;
  if (C % 32 != 0 || C > 256 || Hd % 64 != 0 || Hd > 1024) return BEVOPS_NOT_SUPPORTED;
  if (Dz > 16 || Ncls > 32 || Dz * Ncls > 320) return BEVOPS_NOT_SUPPORTED;
  const long long rows = (long long)B * H * W;
  if ((long long)H * W > 0x7fffffffLL || rows > 0x7fffffffLL * (long long)kOccRows / 2) return BEVOPS_NOT_SUPPORTED;
  if (rows == 0) return BEVOPS_SUCCESS;
  OccArgs p;
  p.y = static_cast<const __half *>(y); p.w1 = static_cast<const __half *>(w1); p.b1 = static_cast<const __half *>(b1);
  p.w2 = static_cast<const __half *>(w2_packed); p.b2 = static_cast<const __half *>(b2_packed);
  p.occ = static_cast<unsigned char *>(occ); p.logits = static_cast<__half *>(logits);
  p.rows = rows; p.s_img = occ_stride_image; p.s_line = occ_stride_line; p.s_px = occ_stride_pixel;
  p.y_pitch = y_pitch; p.C = C; p.Hd = Hd; p.Dz = Dz; p.Ncls = Ncls; p.H = H; p.W = W;
  p.nb = bevops_occ_head_blocks(Dz, Ncls);
  p.vec16 = Dz == 16 && !misaligned(occ, 15u) && occ_stride_image % 16 == 0 && occ_stride_line % 16 == 0 &&
            occ_stride_pixel % 16 == 0;
  if (!ensure_dynamic_lds<occ_head_kernel>(kOccLds)) return BEVOPS_FAILURE;
  hipLaunchKernelGGL(occ_head_kernel, dim3((unsigned)((rows + kOccRows - 1) / kOccRows)), dim3(256), kOccLds,
                     static_cast<hipStream_t>(stream), p);
  return launch_status();
}
