// Grouped, UNMODULATED deformable convolution (DCNv1: mmcv's `DCN` pack as BEVDepth's DepthNet uses it, groups = 4,
// deform_groups = 1): 3 x 3, stride 1, padding 1, dilation 1, channels-last fp16.  design/bevdepth_dcn.md.
//
// One launch for all groups, no workspace, no atomics.  Block (tile, y) with y = group * cblocks + cblock owns 64
// consecutive pixels of the flattened [B * H * W] pixel axis and up to 64 output channels of ONE conv group; its four
// waves are 2 (32-pixel halves) x 2 (32-channel halves).  A wave whose 32 channels lie behind Cout / groups issues no
// matrix-core pass: a group's output rows are padded to 32, never further.
//
// k order: tap (row-major) outermost, then the group's input channels in chunks of KC (64 when Cin / groups is a
// multiple of 64, else 32).  Per step the 256 threads
//   * sample the tile's [64 pixels][KC channels] operand: thread = (pixel, 8 or 16 channels); position
//     h = y - 1 + i + off_h, w = x - 1 + j + off_w in fp32 from the fp16 offsets; the tap is live iff h > -1 && w > -1
//     && h < H && w < W; every corner inside the image is loaded (16-byte vectors) and multiplied, even by a zero
//     weight; a corner outside the image is not read and contributes +0;
//         s = w00 * v00;  s = fma(w01, v01, s);  s = fma(w10, v10, s);  s = fma(w11, v11, s)      (fp32)
//     rounded ONCE to fp16 into LDS;
//   * copy the [64 channels][KC] slice of the packed weight ([Cout][tap][Cin / groups], bevops_mdconv_pack_weight)
//     into LDS;
// and each wave runs KC / 16 v_mfma_f32_32x32x16_f16 passes (A = weights, B = samples, fp32 accumulators).  The global
// loads of step s + 1 are issued before the passes of step s and land in registers.
// Epilogue: acc + bias in fp32, optional ReLU, ONE rounding to fp16, through LDS into whole 16-byte channel vectors.
//
// LDS rows carry 8 halves of padding (row strides of 144 / 80 bytes = 36 / 20 dwords): the 16 rows a ds_read_b128 lane
// group touches start on 16 different 16-byte slots of the 64-bank row.
#include "common.h"

namespace bevops {
namespace {

typedef _Float16 dfc_f16x8 __attribute__((ext_vector_type(8)));
typedef float dfc_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kDfcPix = 64;                  // pixels of a block
constexpr int kDfcCo = 64;                   // output channels of a block
constexpr int kDfcThreads = 256;
constexpr int kDfcTaps = 9;
constexpr int kDfcPad = 8;                   // halves of row padding in LDS

struct DfcDims {
  int H, W, Cin, Cout, cin_g, cout_g, cblocks, offset_channels, relu;
  int N;                                     // B * H * W
};

template <int KC>
__global__ __launch_bounds__(kDfcThreads) void deform_conv3x3_f16_kernel(const __half *__restrict__ x,
                                                                          const __half *__restrict__ offset,
                                                                          const __half *__restrict__ wpk,
                                                                          const __half *__restrict__ bias,
                                                                          __half *__restrict__ out, DfcDims d) {
  constexpr int LD = KC + kDfcPad;           // halves per LDS operand row
  constexpr int VPT = KC / 32;               // 16-byte vectors per thread and operand row
  constexpr int OLD = kDfcCo + kDfcPad;      // halves per row of the output image
  constexpr int kOperand = kDfcPix * LD;     // halves of one operand image
  static_assert(2 * kOperand >= kDfcPix * OLD, "the output image reuses the operand images");
  __shared__ __attribute__((aligned(16))) __half smem[2 * kOperand];
  __shared__ unsigned s_off[kDfcPix * kDfcTaps];     // (off_h, off_w) fp16 pairs, [pixel][tap]
  __half *sA = smem, *sB = smem + kOperand;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pw = wave & 1, cw = wave >> 1;
  const int g = blockIdx.y / d.cblocks, cblk = blockIdx.y - g * d.cblocks;
  const int n0 = blockIdx.x * kDfcPix;               // n0 + 63 < 2^31: checked by the entry
  const int HW = d.H * d.W;

  for (int i = tid; i < kDfcPix * kDfcTaps; i += kDfcThreads) {
    const int p = i / kDfcTaps, t = i - p * kDfcTaps;
    unsigned v = 0u;
    if (n0 + p < d.N) v = *reinterpret_cast<const unsigned *>(offset + (size_t)(n0 + p) * d.offset_channels + 2 * t);
    s_off[i] = v;
  }

  // this thread's operand row: pixel `row` of the tile for the samples, channel `row` of the block for the weights
  const int row = tid >> 2, v0 = (tid & 3) * VPT;
  const int n = n0 + row;
  const bool pvalid = n < d.N;
  const int img = pvalid ? n / HW : 0;
  const int rem = pvalid ? n - img * HW : 0;
  const int py = rem / d.W, px = rem - py * d.W;
  const __half *ximg = x + (size_t)img * HW * d.Cin + (size_t)g * d.cin_g;
  const int co_row = cblk * kDfcCo + row;            // channel inside the group
  const bool wvalid = co_row < d.cout_g;
  const __half *wrow = wpk + (size_t)(g * d.cout_g + (wvalid ? co_row : 0)) * kDfcTaps * d.cin_g;

  const int chunks = d.cin_g / KC, steps = kDfcTaps * chunks;
  uint4 rc[4][VPT], rw[VPT];
  float cwgt[4];
  auto fetch = [&](int tap, int chunk) {
    const unsigned o2 = s_off[row * kDfcTaps + tap];
    const float off_h = h2f_lo(o2), off_w = h2f_hi(o2);
    const int i = tap / 3, j = tap - i * 3;
    float h_im = (float)(py - 1 + i) + off_h, w_im = (float)(px - 1 + j) + off_w;
    const bool in = pvalid && h_im > -1.f && w_im > -1.f && h_im < (float)d.H && w_im < (float)d.W;
    if (!in) h_im = 0.f, w_im = 0.f;
    const float hf = floorf(h_im), wf = floorf(w_im);
    const int h0 = (int)hf, w0 = (int)wf;
    const float lh = h_im - hf, lw = w_im - wf, hh = 1.f - lh, hw = 1.f - lw;
    const float wq[4] = {hh * hw, hh * lw, lh * hw, lh * lw};
    const int hs[4] = {h0, h0, h0 + 1, h0 + 1}, ws[4] = {w0, w0 + 1, w0, w0 + 1};
    const int c0 = chunk * KC + v0 * 8;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool ok = in && hs[q] >= 0 && hs[q] <= d.H - 1 && ws[q] >= 0 && ws[q] <= d.W - 1;
      cwgt[q] = ok ? wq[q] : 0.f;
      const __half *src = ximg + (size_t)(ok ? hs[q] * d.W + ws[q] : 0) * d.Cin + c0;
#pragma unroll
      for (int v = 0; v < VPT; ++v) rc[q][v] = ok ? *reinterpret_cast<const uint4 *>(src + v * 8) : make_uint4(0u, 0u, 0u, 0u);
    }
    const __half *wsrc = wrow + (size_t)tap * d.cin_g + c0;
#pragma unroll
    for (int v = 0; v < VPT; ++v) rw[v] = wvalid ? *reinterpret_cast<const uint4 *>(wsrc + v * 8) : make_uint4(0u, 0u, 0u, 0u);
  };
  auto blend = [&](unsigned a, unsigned b, unsigned c, unsigned e) -> unsigned {
    float lo = cwgt[0] * h2f_lo(a), hi = cwgt[0] * h2f_hi(a);
    lo = fmaf(cwgt[1], h2f_lo(b), lo); hi = fmaf(cwgt[1], h2f_hi(b), hi);
    lo = fmaf(cwgt[2], h2f_lo(c), lo); hi = fmaf(cwgt[2], h2f_hi(c), hi);
    lo = fmaf(cwgt[3], h2f_lo(e), lo); hi = fmaf(cwgt[3], h2f_hi(e), hi);
    return pack_h2(lo, hi);
  };
  auto stage = [&]() {
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
      uint4 s;
      s.x = blend(rc[0][v].x, rc[1][v].x, rc[2][v].x, rc[3][v].x);
      s.y = blend(rc[0][v].y, rc[1][v].y, rc[2][v].y, rc[3][v].y);
      s.z = blend(rc[0][v].z, rc[1][v].z, rc[2][v].z, rc[3][v].z);
      s.w = blend(rc[0][v].w, rc[1][v].w, rc[2][v].w, rc[3][v].w);
      *reinterpret_cast<uint4 *>(sB + row * LD + (v0 + v) * 8) = s;
      *reinterpret_cast<uint4 *>(sA + row * LD + (v0 + v) * 8) = rw[v];
    }
  };

  dfc_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const bool active = cblk * kDfcCo + cw * 32 < d.cout_g;      // wave-uniform
  const int fr = lane & 31, fh = lane >> 5;
  const __half *fa = sA + (cw * 32 + fr) * LD + fh * 8;
  const __half *fb = sB + (pw * 32 + fr) * LD + fh * 8;

  __syncthreads();                                             // s_off
  fetch(0, 0);
  int tap = 0, chunk = 0;
  for (int s = 0; s < steps; ++s) {
    stage();
    __syncthreads();
    if (++chunk == chunks) { chunk = 0; ++tap; }
    if (s + 1 < steps) fetch(tap, chunk);
    if (active) {
#pragma unroll
      for (int ks = 0; ks < KC / 16; ++ks) {
        const dfc_f16x8 a = *reinterpret_cast<const dfc_f16x8 *>(fa + ks * 16);
        const dfc_f16x8 b = *reinterpret_cast<const dfc_f16x8 *>(fb + ks * 16);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // acc[4 q + i]: channel cw * 32 + 8 q + 4 fh + i of the block, pixel pw * 32 + fr
  __half *sO = smem;
  if (active) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cl = cw * 32 + 8 * q + 4 * fh;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = acc[4 * q + i];
        if (bias) v[i] = add_rn(v[i], __half2float(bias[g * d.cout_g + cblk * kDfcCo + cl + i]));
        if (d.relu) v[i] = fmaxf(v[i], 0.f);
      }
      uint2 o;
      o.x = pack_h2(v[0], v[1]);
      o.y = pack_h2(v[2], v[3]);
      *reinterpret_cast<uint2 *>(sO + (pw * 32 + fr) * OLD + cl) = o;
    }
  }
  __syncthreads();
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const int cl = ((tid & 3) * 2 + v) * 8;                    // 8 channels: all inside the group or all behind it
    if (pvalid && cblk * kDfcCo + cl < d.cout_g)
      *reinterpret_cast<uint4 *>(out + (size_t)n * d.Cout + g * d.cout_g + cblk * kDfcCo + cl) =
          *reinterpret_cast<const uint4 *>(sO + row * OLD + cl);
  }
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_deform_conv3x3_nhwc_f16(const void *input_nhwc, const void *offset_nhwc, int offset_channels,
                                              const void *packed_weight, const void *bias, void *output_nhwc, int relu,
                                              int B, int H, int W, int Cin, int Cout, int groups, void *stream) {
  if (!input_nhwc || !offset_nhwc || !packed_weight || !output_nhwc) return BEVOPS_BAD_PARAM;
  if (!aligned16(input_nhwc) || !aligned16(offset_nhwc) || !aligned16(packed_weight) || !aligned16(output_nhwc) ||
      (bias && !aligned16(bias)))
    return BEVOPS_BAD_PARAM;
  if (B < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || groups <= 0 || (relu != 0 && relu != 1)) return BEVOPS_BAD_PARAM;
  if (offset_channels < 2 * kDfcTaps || (offset_channels & 1)) return BEVOPS_BAD_PARAM;
  if (Cin % groups || Cout % groups) return BEVOPS_NOT_SUPPORTED;
  const int cin_g = Cin / groups, cout_g = Cout / groups;
  if (cin_g % 32 || cout_g % 32) return BEVOPS_NOT_SUPPORTED;
  const int cblocks = (cout_g + kDfcCo - 1) / kDfcCo;
  const unsigned long long pixels = (unsigned long long)B * H * W;
  if (pixels > 0x7fffffffull - kDfcPix || (unsigned long long)H * W > 0x7fffffffull) return BEVOPS_NOT_SUPPORTED;
  if ((unsigned long long)groups * cblocks > 65535ull) return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  const DfcDims d{H, W, Cin, Cout, cin_g, cout_g, cblocks, offset_channels, relu, (int)pixels};
  const dim3 grid((unsigned)((pixels + kDfcPix - 1) / kDfcPix), (unsigned)(groups * cblocks));
  auto kern = cin_g % 64 == 0 ? deform_conv3x3_f16_kernel<64> : deform_conv3x3_f16_kernel<32>;
  hipLaunchKernelGGL(kern, grid, dim3(kDfcThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const __half *>(input_nhwc), static_cast<const __half *>(offset_nhwc),
                     static_cast<const __half *>(packed_weight), static_cast<const __half *>(bias),
                     static_cast<__half *>(output_nhwc), d);
  return launch_status();
}
