// Grouped, UNMODULATED deformable convolution on channels-last INT8 (bevops_deform_conv3x3_nhwc_s8): the int8 sibling of
// bevops_deform_conv3x3_nhwc_f16 (csrc/deform_conv.hip) for the INT8 build of BEVDepth's DepthNet with its DCN layer
// (quantization.build_int8_bevdet(depthnet_dcn="int8")).  3 x 3, stride 1, padding 1, dilation 1, ONE deform group, any
// number of conv groups in ONE launch.  design/bevdepth_dcn_int8.md.
//
// OPERATION ORDER (include/bevops.h repeats it; every step one fp32 operation):
//   positions   h = (float)(y - 1 + i) + (float)off_h, w likewise, from the UN-quantised fp16 offsets; the tap is live iff
//               h > -1 && w > -1 && h < H && w < W (a NaN or infinite offset: dead); lh = h - floorf(h), hh = 1 - lh;
//               corner weights hh hw, hh lw, lh hw, lh lw, one product each; a corner outside the image is not read and
//               contributes +0;
//   sample      s = w00 * (float)v00; s = fma(w01, (float)v01, s); s = fma(w10, (float)v10, s); s = fma(w11, (float)v11, s);
//               column byte c = min(max(rne(s), -127), 127): the column keeps the INPUT's scale (bilinear interpolation is
//               convex), there is no second scale and there are no 8-bit area weights;
//   sum         sum = sum over (tap, channel of the group) of c * w_q: exact int32 on v_mfma_i32_32x32x32_i8;
//   epilogue    bevops_conv_slice_s8's, without an identity: sc = (scale_a * scale_w) * w_scales[co] (the product in
//               parentheses on the host), v = fma((float)sum, sc, bias[co]), ReLU, then
//               int8: min(max(rne(v * inv), -127), 127), inv = 1.f / scale_out on the host (a NaN leaves as -127);
//               fp16: one rounding.
//
// MI355X mapping: deform_conv.hip's.  Block (tile, y) with y = group * cblocks + cblock owns 64 consecutive pixels of the
// flattened [B * H * W] pixel axis and up to 64 output channels of ONE group; four waves = 2 (32-pixel halves) x 2
// (32-channel halves); a wave whose 32 channels lie behind Cout / groups issues no matrix pass.  k order: tap (row-major)
// outermost, then the group's channels in chunks of KC bytes (64 when Cin / groups is a multiple of 64, else 32).  Thread
// t owns operand row t >> 2 and the 16-byte vector t & 3 of the chunk (KC = 32: vectors 0 and 1; the other two threads of
// the row move nothing): four 16-byte corner loads, 16 channels blended, one 16-byte LDS store; the weight vector of
// channel row t >> 2 likewise.  The global loads of step s + 1 are issued before the matrix passes of step s.
// LDS rows carry 16 bytes of padding (row strides of 80 / 48 bytes = 20 / 12 dwords: odd multiples of a 16-byte slot), so
// the 16 rows a ds_read_b128 lane group touches start on 16 different slots of the 64-bank row.
// The epilogue goes through LDS into whole 16-byte channel vectors.  Every byte offset is 64-bit.
#include "common.h"
#include "gemm_host.h"

namespace bevops {
namespace {

typedef int dfq_i32x4 __attribute__((ext_vector_type(4)));
typedef int dfq_i32x16 __attribute__((ext_vector_type(16)));

constexpr int kDfqPix = 64;                  // pixels of a block
constexpr int kDfqCo = 64;                   // output channels of a block
constexpr int kDfqThreads = 256;
constexpr int kDfqTaps = 9;
constexpr int kDfqPad = 16;                  // bytes of row padding in LDS

struct DfqDims {
  int H, W, cin_g, cout_g, cblocks, offset_channels, relu;
  int x_pitch, out_pitch;                    // elements between two pixels
  int N;                                     // B * H * W
  float s_aw, inv_s_out;
};

__device__ __forceinline__ float dfq_byte(unsigned w, int k) {      // signed byte k of a word, as fp32 (exact)
  return (float)((int)(w << (24 - 8 * k)) >> 24);
}

__device__ __forceinline__ unsigned dfq_q8(float v) {               // min(max(rne(v), -127), 127) as a byte
  return (unsigned)(int)fminf(fmaxf(rintf(v), -127.f), 127.f) & 0xffu;
}

template <int KC, bool OUT8>
__global__ __launch_bounds__(kDfqThreads) void deform_conv3x3_s8_kernel(const signed char *__restrict__ x,
                                                                         const __half *__restrict__ offset,
                                                                         const signed char *__restrict__ wq,
                                                                         const float *__restrict__ wscale,
                                                                         const float *__restrict__ bias,
                                                                         void *__restrict__ out, DfqDims d) {
  constexpr int LD = KC + kDfqPad;                               // bytes per LDS operand row
  constexpr int VEC = KC / 16;                                   // 16-byte vectors per operand row
  constexpr int OLD = OUT8 ? kDfqCo + 16 : (kDfqCo + 8) * 2;     // bytes per row of the output image
  constexpr int kOperand = kDfqPix * LD;                         // bytes of one operand image
  constexpr int kSmem = 2 * kOperand > kDfqPix * OLD ? 2 * kOperand : kDfqPix * OLD;
  __shared__ __attribute__((aligned(16))) char smem[kSmem];
  __shared__ unsigned s_off[kDfqPix * kDfqTaps];                 // (off_h, off_w) fp16 pairs, [pixel][tap]
  char *sA = smem, *sB = smem + kOperand;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pw = wave & 1, cw = wave >> 1;
  const int g = blockIdx.y / d.cblocks, cblk = blockIdx.y - g * d.cblocks;
  const int n0 = blockIdx.x * kDfqPix;                           // n0 + 63 < 2^31: checked by the entry
  const int HW = d.H * d.W;

  for (int i = tid; i < kDfqPix * kDfqTaps; i += kDfqThreads) {
    const int p = i / kDfqTaps, t = i - p * kDfqTaps;
    unsigned v = 0u;
    if (n0 + p < d.N) v = *reinterpret_cast<const unsigned *>(offset + (size_t)(n0 + p) * d.offset_channels + 2 * t);
    s_off[i] = v;
  }

  // this thread's operand row: pixel `row` of the tile for the samples, channel `row` of the block for the weights
  const int row = tid >> 2, vec = tid & 3;
  const bool vact = vec < VEC;                                   // KC = 32: two vectors per row
  const int n = n0 + row;
  const bool pvalid = n < d.N;
  const int img = pvalid ? n / HW : 0;
  const int rem = pvalid ? n - img * HW : 0;
  const int py = rem / d.W, px = rem - py * d.W;
  const signed char *ximg = x + (size_t)img * HW * d.x_pitch + (size_t)g * d.cin_g;
  const int co_row = cblk * kDfqCo + row;                        // channel inside the group
  const bool wvalid = vact && co_row < d.cout_g;
  const signed char *wrow = wq + (size_t)(g * d.cout_g + (wvalid ? co_row : 0)) * kDfqTaps * d.cin_g;

  const int chunks = d.cin_g / KC, steps = kDfqTaps * chunks;
  uint4 rc[4], rw;
  float cwgt[4];
  auto fetch = [&](int tap, int chunk) {
    const unsigned o2 = s_off[row * kDfqTaps + tap];
    const float off_h = h2f_lo(o2), off_w = h2f_hi(o2);
    const int i = tap / 3, j = tap - i * 3;
    float h_im = (float)(py - 1 + i) + off_h, w_im = (float)(px - 1 + j) + off_w;
    const bool in = pvalid && vact && h_im > -1.f && w_im > -1.f && h_im < (float)d.H && w_im < (float)d.W;
    if (!in) h_im = 0.f, w_im = 0.f;
    const float hf = floorf(h_im), wf = floorf(w_im);
    const int h0 = (int)hf, w0 = (int)wf;
    const float lh = h_im - hf, lw = w_im - wf, hh = 1.f - lh, hw = 1.f - lw;
    const float wgt[4] = {hh * hw, hh * lw, lh * hw, lh * lw};
    const int hs[4] = {h0, h0, h0 + 1, h0 + 1}, ws[4] = {w0, w0 + 1, w0, w0 + 1};
    const int c0 = chunk * KC + vec * 16;                        // c0 + 16 <= Cin / groups whenever vact
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool ok = in && hs[q] >= 0 && hs[q] <= d.H - 1 && ws[q] >= 0 && ws[q] <= d.W - 1;
      cwgt[q] = ok ? wgt[q] : 0.f;
      const signed char *src = ximg + (size_t)(ok ? hs[q] * d.W + ws[q] : 0) * d.x_pitch + c0;
      rc[q] = ok ? *reinterpret_cast<const uint4 *>(src) : make_uint4(0u, 0u, 0u, 0u);
    }
    rw = wvalid ? *reinterpret_cast<const uint4 *>(wrow + (size_t)tap * d.cin_g + c0) : make_uint4(0u, 0u, 0u, 0u);
  };
  auto blend = [&](unsigned a, unsigned b, unsigned c, unsigned e) -> unsigned {
    unsigned r = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float s = cwgt[0] * dfq_byte(a, k);
      s = __builtin_fmaf(cwgt[1], dfq_byte(b, k), s);
      s = __builtin_fmaf(cwgt[2], dfq_byte(c, k), s);
      s = __builtin_fmaf(cwgt[3], dfq_byte(e, k), s);
      r |= dfq_q8(s) << (8 * k);
    }
    return r;
  };
  auto stage = [&]() {
    if (!vact) return;
    uint4 s;
    s.x = blend(rc[0].x, rc[1].x, rc[2].x, rc[3].x);
    s.y = blend(rc[0].y, rc[1].y, rc[2].y, rc[3].y);
    s.z = blend(rc[0].z, rc[1].z, rc[2].z, rc[3].z);
    s.w = blend(rc[0].w, rc[1].w, rc[2].w, rc[3].w);
    *reinterpret_cast<uint4 *>(sB + row * LD + vec * 16) = s;
    *reinterpret_cast<uint4 *>(sA + row * LD + vec * 16) = rw;
  };

  dfq_i32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0;
  const bool active = cblk * kDfqCo + cw * 32 < d.cout_g;        // wave-uniform
  const int fr = lane & 31, fh = lane >> 5;
  const char *fa = sA + (cw * 32 + fr) * LD + fh * 16;
  const char *fb = sB + (pw * 32 + fr) * LD + fh * 16;

  __syncthreads();                                               // s_off
  fetch(0, 0);
  int tap = 0, chunk = 0;
  for (int s = 0; s < steps; ++s) {
    stage();
    __syncthreads();
    if (++chunk == chunks) { chunk = 0; ++tap; }
    if (s + 1 < steps) fetch(tap, chunk);
    if (active) {
#pragma unroll
      for (int ks = 0; ks < KC / 32; ++ks) {
        const dfq_i32x4 a = *reinterpret_cast<const dfq_i32x4 *>(fa + ks * 32);
        const dfq_i32x4 b = *reinterpret_cast<const dfq_i32x4 *>(fb + ks * 32);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // acc[4 q + i]: channel cw * 32 + 8 q + 4 fh + i of the block, pixel pw * 32 + fr
  char *sO = smem;
  const int cobase = g * d.cout_g + cblk * kDfqCo;               // the block's first channel
  if (active) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cl = cw * 32 + 8 * q + 4 * fh;
      float4 sc = make_float4(d.s_aw, d.s_aw, d.s_aw, d.s_aw), bs = make_float4(0.f, 0.f, 0.f, 0.f);
      if (wscale) {
        const float4 w4 = *reinterpret_cast<const float4 *>(wscale + cobase + cl);
        sc = make_float4(mul_rn(d.s_aw, w4.x), mul_rn(d.s_aw, w4.y), mul_rn(d.s_aw, w4.z), mul_rn(d.s_aw, w4.w));
      }
      if (bias) bs = *reinterpret_cast<const float4 *>(bias + cobase + cl);
      float v[4];
      v[0] = __builtin_fmaf((float)acc[4 * q], sc.x, bs.x);
      v[1] = __builtin_fmaf((float)acc[4 * q + 1], sc.y, bs.y);
      v[2] = __builtin_fmaf((float)acc[4 * q + 2], sc.z, bs.z);
      v[3] = __builtin_fmaf((float)acc[4 * q + 3], sc.w, bs.w);
      if (d.relu) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
      }
      char *dst = sO + (pw * 32 + fr) * OLD;
      if constexpr (OUT8) {
        unsigned pk = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) pk |= dfq_q8(mul_rn(v[i], d.inv_s_out)) << (8 * i);
        *reinterpret_cast<unsigned *>(dst + cl) = pk;
      } else {
        uint2 o;
        o.x = pack_h2(v[0], v[1]);
        o.y = pack_h2(v[2], v[3]);
        *reinterpret_cast<uint2 *>(dst + cl * 2) = o;
      }
    }
  }
  __syncthreads();
  if constexpr (OUT8) {
    const int cl = vec * 16;                                     // 16 channels: all inside the group or all behind it
    if (pvalid && cblk * kDfqCo + cl < d.cout_g)
      *reinterpret_cast<uint4 *>(static_cast<signed char *>(out) + (size_t)n * d.out_pitch + cobase + cl) =
          *reinterpret_cast<const uint4 *>(sO + row * OLD + cl);
  } else {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int cl = (vec * 2 + v) * 8;                          // 8 channels: all inside the group or all behind it
      if (pvalid && cblk * kDfqCo + cl < d.cout_g)
        *reinterpret_cast<uint4 *>(static_cast<__half *>(out) + (size_t)n * d.out_pitch + cobase + cl) =
            *reinterpret_cast<const uint4 *>(sO + row * OLD + cl * 2);
    }
  }
}

}  // namespace
}  // namespace bevops

using namespace bevops;

extern "C" int bevops_deform_conv3x3_nhwc_s8(const void *x_q, int x_pitch, float scale_a, const void *offset_nhwc_f16,
                                             int offset_channels, const void *w_q_taps, const float *w_scales,
                                             float scale_w, const float *bias, int out_dtype, void *out, int out_pitch,
                                             float scale_out, int relu, int B, int H, int W, int Cin, int Cout,
                                             int groups, void *stream) {
  if (!x_q || !offset_nhwc_f16 || !w_q_taps || !out) return BEVOPS_BAD_PARAM;
  if (!aligned16(x_q) || !aligned16(offset_nhwc_f16) || !aligned16(w_q_taps) || !aligned16(out) ||
      (w_scales && !aligned16(w_scales)) || (bias && !aligned16(bias)))
    return BEVOPS_BAD_PARAM;
  if (B < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || groups <= 0 || (relu != 0 && relu != 1)) return BEVOPS_BAD_PARAM;
  if (offset_channels < 2 * kDfqTaps || (offset_channels & 1)) return BEVOPS_BAD_PARAM;
  if (x_pitch < Cin || x_pitch % 16 != 0) return BEVOPS_BAD_PARAM;
  // (16-byte output vectors: 8 elements of fp16, 16 of int8 -- and of a dtype the next check refuses)
  if (out_pitch < Cout || out_pitch % (out_dtype == BEVOPS_F16 ? 8 : 16) != 0) return BEVOPS_BAD_PARAM;
  if (bad_scale(scale_a) || bad_scale(scale_w) || (out_dtype == BEVOPS_I8 && bad_scale(scale_out)))
    return BEVOPS_BAD_PARAM;
  if (out_dtype != BEVOPS_I8 && out_dtype != BEVOPS_F16) return BEVOPS_NOT_SUPPORTED;
  const bool out8 = out_dtype == BEVOPS_I8;
  if (Cin % groups || Cout % groups) return BEVOPS_NOT_SUPPORTED;
  const int cin_g = Cin / groups, cout_g = Cout / groups;
  if (cin_g % 32 || cout_g % 32) return BEVOPS_NOT_SUPPORTED;
  const int cblocks = (cout_g + kDfqCo - 1) / kDfqCo;
  const unsigned long long pixels = (unsigned long long)B * H * W;
  if (pixels > 0x7fffffffull - kDfqPix || (unsigned long long)H * W > 0x7fffffffull) return BEVOPS_NOT_SUPPORTED;
  if ((unsigned long long)groups * cblocks > 65535ull) return BEVOPS_NOT_SUPPORTED;
  if (B == 0) return BEVOPS_SUCCESS;
  const DfqDims d{H, W, cin_g, cout_g, cblocks, offset_channels, relu, x_pitch, out_pitch, (int)pixels,
                  scale_a * scale_w, out8 ? 1.f / scale_out : 1.f};
  const dim3 grid((unsigned)((pixels + kDfqPix - 1) / kDfqPix), (unsigned)(groups * cblocks));
  const bool k64 = cin_g % 64 == 0;
  auto kern = out8 ? (k64 ? deform_conv3x3_s8_kernel<64, true> : deform_conv3x3_s8_kernel<32, true>)
                   : (k64 ? deform_conv3x3_s8_kernel<64, false> : deform_conv3x3_s8_kernel<32, false>);
  hipLaunchKernelGGL(kern, grid, dim3(kDfqThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const signed char *>(x_q), static_cast<const __half *>(offset_nhwc_f16),
                     static_cast<const signed char *>(w_q_taps), w_scales, bias, out, d);
  return launch_status();
}
