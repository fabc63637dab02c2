/*
 * bevops.h -- C ABI of libbevops_hip.so: MI355X (gfx950) HIP kernels for the
 * BEVFormer / BEVDet sampling hot path.
 *
 * This is the drop-in boundary.  Every entry point replaces the device side of
 * one TensorRT plugin of the reference (DerryHub/BEVFormer_tensorrt), i.e. what
 * `IPluginV2DynamicExt::enqueue(inputDesc, outputDesc, inputs, outputs,
 * workspace, stream)` did there; the tensor descriptors are flattened into
 * plain ints/floats.  The reference interface each function replaces is cited
 * as file:line relative to the reference tree.
 *
 * Conventions (restating the reference's, TensorRT/common/helper.h:19-25 and
 * SURVEY.md section 8b):
 *   - return value: bevops_status_t (0 = success).  Never aborts, exits or
 *     throws across the ABI; launch errors are returned, not printed.
 *   - all pointers are DEVICE pointers unless the name ends in `_host`.
 *   - the caller owns every buffer (inputs, outputs, workspace); the library
 *     allocates no device memory.  Process state it DOES keep, all of it
 *     invisible in results: (1) per kernel instance, the dynamic-LDS limit it
 *     has already raised on a device; (2) bevops_linear_*: one hipBLASLt handle
 *     per device and the algorithm chosen per problem, under a mutex (as the
 *     reference keeps the cuBLAS handle TensorRT attaches,
 *     modulatedDeformableConv2dPlugin.cpp:286-290); (3) the `*_set_variant`
 *     A/B hooks (thread-local, default 0 = automatic choice; tests and probes
 *     only).  Every operator entry is re-entrant from several host threads.
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as
 *     void*; NULL = the default stream).  No operator synchronises the host or
 *     is illegal under stream capture; the ONE blocking entry is the optional
 *     tuning call bevops_linear_tune, which says so.
 *   - tensors are dense, row-major ("kLINEAR"), 16-byte aligned.
 *   - dtype enums: BEVOPS_F32 / BEVOPS_F16 / BEVOPS_I8.  INT8 tensors carry a
 *     per-tensor scale (real = int8 * scale), as TensorRT's
 *     PluginTensorDesc::scale did.
 */
#ifndef BEVOPS_H_
#define BEVOPS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  BEVOPS_SUCCESS = 0,         /* STATUS_SUCCESS          helper.h:20 */
  BEVOPS_FAILURE = 1,         /* STATUS_FAILURE          helper.h:21 */
  BEVOPS_BAD_PARAM = 2,       /* STATUS_BAD_PARAM        helper.h:22 */
  BEVOPS_NOT_SUPPORTED = 3,   /* STATUS_NOT_SUPPORTED    helper.h:23 */
  BEVOPS_NOT_INITIALIZED = 4  /* STATUS_NOT_INITIALIZED  helper.h:24 */
} bevops_status_t;

typedef enum { BEVOPS_F32 = 0, BEVOPS_F16 = 1, BEVOPS_I8 = 2, BEVOPS_U8 = 3 /* raw camera images only */ } bevops_dtype_t;

/* interpolation / padding enums: functions/grid_sampler.py:134-136,
 * gridSamplerKernel.h:9-12 */
typedef enum { BEVOPS_BILINEAR = 0, BEVOPS_NEAREST = 1, BEVOPS_BICUBIC = 2 } bevops_interp_t;
typedef enum { BEVOPS_PAD_ZEROS = 0, BEVOPS_PAD_BORDER = 1, BEVOPS_PAD_REFLECTION = 2 } bevops_pad_t;

/* Library identification. */
const char *bevops_version(void);
/* Human-readable text for a status code (static storage). */
const char *bevops_status_string(int status);
/* Address of an entry point by plugin/op name, or NULL.  Accepts the ABI symbol
 * ("bevops_msda_forward") and the reference's plugin type names
 * ("MultiScaleDeformableAttnTRT", "MultiScaleDeformableAttnTRT2", "RotateTRT",
 * "RotateTRT2", "GridSampler2DTRT", "GridSampler2DTRT2", "GridSampler3DTRT",
 * "GridSampler3DTRT2", "BEVPoolV2TRT", "BEVPoolV2TRT2", "ModulatedDeformableConv2dTRT",
 * "ModulatedDeformableConv2dTRT2", "QKVTRT", "QKVTRT2", "InverseTRT";
 * multiScaleDeformableAttnPlugin.cpp:17-18 etc.), standing in for
 * TensorRT's plugin-creator registry (REGISTER_TENSORRT_PLUGIN,
 * multiScaleDeformableAttnPlugin.cpp:345-346). */
void *bevops_query(const char *name);

/* ------------------------------------------------------------------------
 * Multi-scale deformable attention, fused softmax + sampling + weighted sum.
 * Replaces MultiScaleDeformableAttnPlugin::enqueue
 *   (TensorRT/plugin/multi_scale_deformable_attn/multiScaleDeformableAttnPlugin.cpp:71-140)
 * and the launchers ms_deformable_im2col_cuda{,_h2,_int8}
 *   (multiScaleDeformableAttnKernel.h:12-38, multiScaleDeformableAttnKernel.cu:1106-1218).
 *
 *   value            [bs, nk, heads, channels]       dtype
 *   spatial_shapes   [num_levels, 2] int32 (h, w)    device
 *   spatial_shapes_host  same values on the host, or NULL (enables the
 *                    host-side shape check nk == sum h*w; never required)
 *   reference_points [bs, num_query, 1, 2*points_per_group]  ref_dtype (F32|F16);
 *                    must equal dtype for F32/F16 values, either for I8
 *                    (supportsFormatCombination, ...Plugin.cpp:148-189)
 *   sampling_offsets [bs, num_query, heads, num_levels*num_point*2]  dtype
 *   attention_weights[bs, num_query, heads, num_levels*num_point]    dtype, PRE-softmax
 *   output           [bs, num_query, heads, channels] dtype
 *   scale_*          INT8 per-tensor scales (ignored otherwise)
 * INT8 requires channels % 4 == 0 and num_point % 4 == 0 (...Plugin.cpp:151-156),
 * else BEVOPS_NOT_SUPPORTED.  With I8 values, ref_dtype F32 selects the signed
 * x127 weight flavour (kernel.cu:848-955), F16 the unsigned x255 flavour
 * (kernel.cu:957-1104).
 * ------------------------------------------------------------------------ */
int bevops_msda_forward(int dtype, const void *value, const int32_t *spatial_shapes,
                        const int32_t *spatial_shapes_host, const void *reference_points,
                        int ref_dtype, const void *sampling_offsets,
                        const void *attention_weights, void *output, int bs, int nk,
                        int heads, int channels, int num_levels, int num_query,
                        int num_point, int points_per_group, float scale_value,
                        float scale_offset, float scale_weight, float scale_out,
                        void *stream);

/* Same op with a caller-owned scratch buffer (TensorRT's `workspace` argument of enqueue):
 * lets the library re-lay `value` out head-major ([bs][heads][keys][32]) so that the two
 * x-corners of a sample share one cache line and each XCD's L2 holds the (camera, head)
 * plane it gathers from.  bevops_msda_workspace_size returns the bytes required (0 = the
 * path does not apply: channels != 32, ...); a NULL / too small workspace, or one that is not
 * 128-BYTE ALIGNED, simply selects the layout-preserving kernels (a family forced with
 * bevops_msda_set_variant returns BEVOPS_NOT_SUPPORTED instead), results are identical within
 * fp32 rounding.  The library writes inside the first bevops_msda_workspace_size[_shapes] bytes only.
 * For BEVOPS_I8 this query is an UPPER BOUND of the exact, shape-aware size: 3 nk + 3 num_levels + 4
 * entries of 128 bytes per (batch, head) plane, plus 4096.
 * shared_offsets = 1: sampling_offsets / attention_weights are [1, num_query, heads, .] and
 * apply to every one of the bs value batches (BEVFormer's SCA repeats the same query for
 * all cameras, det2trt/models/modules/spatial_cross_attention.py:254) -- identical result
 * to passing them repeated bs times, without the 6x redundant HBM reads. */
size_t bevops_msda_workspace_size(int dtype, int bs, int nk, int heads, int channels,
                                  int num_levels, int num_query, int num_point);
/* Same, for a caller that knows the level shapes on the host ([num_levels][2] = (H, W)):
 * also covers the zero-padded re-layout with LDS-resident small levels (msda_hm3.hip), whose
 * size depends on the level shapes.  BEVOPS_F16: the largest need of every family that may serve
 * the call, >= bevops_msda_workspace_size.  BEVOPS_I8: the exact size of the padded planes,
 * <= bevops_msda_workspace_size (0: the shape is outside the head-major domain). */
size_t bevops_msda_workspace_size_shapes(int dtype, const int32_t *spatial_shapes_host, int bs,
                                         int nk, int heads, int channels, int num_levels,
                                         int num_query, int num_point);
int bevops_msda_forward_ws(int dtype, const void *value, const int32_t *spatial_shapes,
                           const int32_t *spatial_shapes_host, const void *reference_points,
                           int ref_dtype, const void *sampling_offsets,
                           const void *attention_weights, void *output, int bs, int nk,
                           int heads, int channels, int num_levels, int num_query,
                           int num_point, int points_per_group, float scale_value,
                           float scale_offset, float scale_weight, float scale_out,
                           int shared_offsets, void *workspace, size_t workspace_bytes,
                           void *stream);

/* Tuning hook: selects an internal MSDA kernel variant for subsequent calls from
 * this thread (0 = automatic).  Results are identical across variants; exists so
 * tests / tuning scripts can A/B a default against its partner in one process.  The complete list (decoded in
 * csrc/msda.hip: bevops_msda_set_variant, the only place that knows the numbers).  A value that is not on the list
 * selects the automatic choice, exactly as 0 does, and is handed back as it was given by the next call:
 *    1, 2     other point-splits of the layout-preserving quad kernel;   99  the one-thread-per-output generic kernel
 *    10       never a head-major kernel (what multi_scale_deformable_attn_local uses)
 *    11 / 15  head-major generations hm / hm2 forced;  16  hm3;  17  hm4 wherever it is instantiated
 *    19       int8 hm4 on the one-block-per-CU plan (partner of the default two-blocks plan)
 *    1000 / 1001  the fp16 SCA sampler hm5 with / without its visibility pre-pass
 *    3001 .. 3008 slices per CU of the planned fused SCA sampling (default 2; sticky until set again)
 *    3010 / 3011  camera reduce of the fused SCA op with its camera loop unrolled (default) / rolled (sticky)
 *    3012 / 3013  planned fused SCA sampling stores the pairs only one camera sees straight into the output and the
 *                 reduce skips those rows (default) / every pair through the per-camera scratch (sticky)
 *    3014 / 3015  planned fused SCA sampling with the DPP broadcasts of the sample records folded into the instructions
 *                 that consume them and the LDS row taps fused (default, round 6) / the round-5 build (sticky); same bits
 * (The measured-and-rejected builds of rounds 1-4 -- LDS-staged hm, two-copy hm, hm4 chunk sizes / schedule ablations,
 * int8 pixel-pair entries, hm5 with 768 threads / mailbox / persistent blocks / level-class split -- are no longer in
 * the library; their measurements are under profiles/.)  A packed value (bevops_msda_pack_value) must be sampled under
 * the variant it was packed under.  Returns the previously REQUESTED kernel-family value; the 30xx knobs are independent
 * of the family selection: they are neither recorded as, nor returned as, the requested value, so
 * `prev = set_variant(10); ...; set_variant(prev)` restores the family whatever 30xx calls came before or in between. */
int bevops_msda_set_variant(int variant);


/* ------------------------------------------------------------------------
 * rotate: img [channels, height, width] rotated by *angle degrees (counter-clockwise)
 * about *center (x, y in pixels); zeros padding, align_corners = false.
 * Replaces RotatePlugin::enqueue (TensorRT/plugin/rotate/rotatePlugin.cpp:75-116) and
 * rotate<T> / rotate_h2 / rotate_int8 (rotateKernel.h:14-26, rotateKernel.cu:708-748).
 *   angle  : 1 element, center : 2 elements, DEVICE memory, angle_dtype F32|F16
 *            (F32 images need F32 angle/center, rotatePlugin.cpp:125-156)
 *   interpolation : BEVOPS_BILINEAR | BEVOPS_NEAREST
 *   I8 : dense [C,H,W] int8 (the reference used kCHW4), real = int8 * scale_in;
 *        output requantised with scale_out.
 * ------------------------------------------------------------------------ */
int bevops_rotate_forward(int dtype, const void *img, const void *angle, const void *center,
                          int angle_dtype, void *output, int channels, int height, int width,
                          int interpolation, float scale_in, float scale_out, void *stream);

/* ------------------------------------------------------------------------
 * grid_sampler, 2-D: input [N,C,H_in,W_in], grid [N,2,H_out,W_out] channel-first
 * (x, y) in [-10, 10] units, output [N,C,H_out,W_out]; all of dtype.
 * Replaces GridSamplerPlugin::enqueue (TensorRT/plugin/grid_sampler/gridSamplerPlugin.cpp:110-156),
 * grid_sample<T> and grid_sample_int8 (gridSamplerKernel.h:14-26, gridSamplerKernel.cu:1933-2043).
 *   interpolation : bilinear | nearest | bicubic;  padding : zeros | border | reflection
 *   I8 : all three interpolation modes; grid is int8 with scale_grid.
 * 3-D: input [N,C,D,H,W], grid [N,3,D_out,H_out,W_out] (x, y, z); F32 / F16;
 *      bilinear (trilinear) | nearest.
 * ------------------------------------------------------------------------ */
int bevops_grid_sampler_2d_forward(int dtype, const void *input, const void *grid, void *output,
                                   int N, int C, int H_in, int W_in, int H_out, int W_out,
                                   int interpolation, int padding, int align_corners,
                                   float scale_in, float scale_grid, float scale_out,
                                   void *stream);
/* bevops_grid_sampler_2d_forward with a caller-lent scratch buffer (mirrors getWorkspaceSize): fp32 /
 * fp16 bilinear / nearest calls with C % 8 == 0 whose output is >= 2x the input stage the input
 * channels-last in the workspace (one 16-byte load per tap and 8-channel chunk instead of 8 two-byte
 * gathers); every other call runs the planar kernel.  Results are bit-identical either way.
 * bevops_grid_sampler_2d_workspace_size: bytes to lend (0 = the staged path does not apply). */
size_t bevops_grid_sampler_2d_workspace_size(int dtype, int N, int C, int H_in, int W_in);
int bevops_grid_sampler_2d_forward_ws(int dtype, const void *input, const void *grid, void *output,
                                      int N, int C, int H_in, int W_in, int H_out, int W_out,
                                      int interpolation, int padding, int align_corners,
                                      float scale_in, float scale_grid, float scale_out,
                                      void *workspace, size_t workspace_bytes, void *stream);
int bevops_grid_sampler_3d_forward(int dtype, const void *input, const void *grid, void *output,
                                   int N, int C, int D_in, int H_in, int W_in, int D_out,
                                   int H_out, int W_out, int interpolation, int padding,
                                   int align_corners, void *stream);

/* ------------------------------------------------------------------------
 * bev_pool_v2 (BEVDet pillar pooling):
 *   out[ranks_bev[s_k], :] = sum_{i < len_k} depth.flat[ranks_depth[s_k+i]] * feat.flat[ranks_feat[s_k+i], :]
 * all other output cells are zero.  Replaces BEVPoolPlugin::enqueue
 * (TensorRT/plugin/bev_pool_v2/bevPoolPlugin.cpp:68-109) and bev_pool_v2 / _h2 / _int8
 * (bevPoolKernel.h:13-31, bevPoolKernel.cu:151-190).
 *   depth  [N,D,H,W] dtype, feat [N,H,W,channels] dtype, ranks_* [n_points] int32,
 *   interval_starts / interval_lengths [n_intervals] int32,
 *   output [1, out_height, out_width, channels] dtype (fully written: cleared on `stream`).
 *   I8: out = T2int8(acc * scale_depth * scale_feat / scale_out), int32 accumulation.
 * ------------------------------------------------------------------------ */
int bevops_bev_pool_v2_forward(int dtype, const void *depth, const void *feat,
                               const int32_t *ranks_depth, const int32_t *ranks_feat,
                               const int32_t *ranks_bev, const int32_t *interval_starts,
                               const int32_t *interval_lengths, void *output, int channels,
                               int n_intervals, int out_height, int out_width,
                               float scale_depth, float scale_feat, float scale_out,
                               void *stream);

/* ---------------------------------------------------------------------------
 * Fused spatial cross-attention sampling.  NOT a reference plugin: it replaces the
 * sequence of det2trt/models/modules/spatial_cross_attention.py:254-270 --
 *   query.repeat(num_cams) -> MultiScaleDeformableAttnTRT on [num_cams, nq, ...] ->
 *   slots = (queries * bev_mask).sum(0)
 * -- with one call that (a) takes the camera-independent sampling_offsets / attention_weights
 * once ([1, nq, heads, L*P*2] / [1, nq, heads, L*P]), (b) skips every (camera, query) pair whose
 * bev_mask weight is 0 (the rebatching of the original PyTorch SCA,
 * third_party/bev_mmdet3d/models/modules/spatial_cross_attention.py:143-191) and (c) returns the
 * masked camera sum  output[q, heads, C] = sum_cam bev_mask[cam, q] * sample(cam, q).
 *   value [num_cams, nk, heads, C] fp16, reference_points_cam [num_cams, nq, 1, 2*ppg] fp16,
 *   bev_mask [num_cams, nq] fp16 (0 = not visible, else the weight), output [nq, heads, C] fp16.
 * F16, C == 32 only (NOT_SUPPORTED otherwise: compose the reference sequence instead).
 * workspace: bevops_sca_workspace_size bytes (0 = unsupported arguments), 128-BYTE ALIGNED; a NULL, misaligned or
 * short one is BEVOPS_BAD_PARAM (this entry has no other kernel to fall back to).
 * ------------------------------------------------------------------------ */
size_t bevops_sca_workspace_size(int dtype, const int32_t *spatial_shapes_host, int num_cams, int nk,
                                 int heads, int channels, int num_levels, int num_query,
                                 int num_point);
int bevops_sca_forward(int dtype, const void *value, const int32_t *spatial_shapes_host,
                       const void *reference_points_cam, const void *sampling_offsets,
                       const void *attention_weights, const void *bev_mask, void *output,
                       int num_cams, int nk, int heads, int channels, int num_levels, int num_query,
                       int num_point, int points_per_group, void *workspace, size_t workspace_bytes,
                       void *stream);

/* ------------------------------------------------------------------------
 * Modulated deformable convolution (DCNv2) forward.
 * Replaces ModulatedDeformableConv2dPlugin::enqueue / getWorkspaceSize
 * (TensorRT/plugin/modulated_deformable_conv2d/modulatedDeformableConv2dPlugin.cpp:73-197)
 * and ModulatedDeformConvForwardCUDAKernel<T> (modulatedDeformableConv2dKernel.h:11-30,
 * modulatedDeformableConv2dKernel.cu:695-978).
 *   input  [B,Cin,H,W], offset [B, deform_groups*2*Kh*Kw, Ho, Wo] (per tap: h then w),
 *   mask   [B, deform_groups*Kh*Kw, Ho, Wo], weight [Cout, Cin/groups, Kh, Kw],
 *   bias   [Cout] or NULL, output [B,Cout,Ho,Wo];  Ho/Wo from the usual conv formula.
 *   workspace: caller-owned scratch of at least bevops_mdconv_workspace_size(...) bytes
 *   (mirrors getWorkspaceSize; 0 = unsupported arguments), 16-byte aligned.
 * F32 and F16 (F16 needs (Cin/groups*Kh*Kw) % 8 == 0) through bevops_mdconv_forward; INT8
 * through bevops_mdconv_forward_int8 (int8 input / offset / mask / weight with per-tensor
 * scales, fp32 bias, int8 output: out = T2int8((acc*scale_in*scale_weight + bias)/scale_out),
 * modulatedDeformableConv2dKernel.cu:463-607,897-978; needs Cin % 4 == 0,
 * (Cout/groups) % 4 == 0 like ...Plugin.cpp:217-219).
 * bevops_mdconv_workspace_size(BEVOPS_I8, ...) sizes its workspace.
 * ------------------------------------------------------------------------ */
/* Tuning hook like bevops_msda_set_variant (thread-local; a value acts on both dtype families):
 *   0 = automatic (fused implicit GEMM when the channel counts allow);
 *   1 / 2 / 3 = fp16 on the im2col + GEMM pipeline / the register-staged fused kernel with 256 / with 512 threads
 *               (int8 stays automatic);
 *   4 = no split-K tail, fp16 also on 64-pixel tiles; 5 = 128-pixel tiles whatever the tile count (fp16 and int8);
 *   6 / 8 / 9 = int8 on the im2col + GEMM pair / the register-staged fused kernel / the LDS-DMA kernel whatever the
 *               tile count (an fp16 call inside the fused domain runs on the 512-thread register-staged kernel, as
 *               under 3).
 * Any other value selects the automatic choice, exactly as 0 does.  Returns the previous value. */
int bevops_mdconv_set_variant(int variant);
size_t bevops_mdconv_workspace_size(int dtype, int B, int Cin, int H, int W, int Cout, int Kh,
                                    int Kw, int stride_h, int stride_w, int pad_h, int pad_w,
                                    int dil_h, int dil_w, int groups, int deform_groups);
int bevops_mdconv_forward_int8(const void *input, float scale_in, const void *offset,
                               float scale_offset, const void *mask, float scale_mask,
                               const void *weight, float scale_weight, const float *bias,
                               void *output, float scale_out, void *workspace,
                               size_t workspace_bytes, int B, int Cin, int H, int W, int Cout, int Kh,
                               int Kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                               int dil_w, int groups, int deform_groups, void *stream);
/* the same with the weights already re-laid-out by bevops_mdconv_pack_weight(BEVOPS_I8, ...) */
int bevops_mdconv_forward_int8_packed(const void *input, float scale_in, const void *offset,
                                      float scale_offset, const void *mask, float scale_mask,
                                      const void *packed_weight, float scale_weight, const float *bias,
                                      void *output, float scale_out, void *workspace,
                                      size_t workspace_bytes, int B, int Cin, int H, int W, int Cout, int Kh,
                                      int Kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                                      int dil_w, int groups, int deform_groups, void *stream);
int bevops_mdconv_forward(int dtype, const void *input, const void *offset, const void *mask,
                          const void *weight, const void *bias, void *output, void *workspace,
                          size_t workspace_bytes, int B, int Cin, int H, int W, int Cout, int Kh,
                          int Kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                          int dil_w, int groups, int deform_groups, void *stream);
/* Inference keeps the same weights call after call: the [Cout][tap][Cin/groups] re-layout that
 * bevops_mdconv_forward makes inside its workspace on every call can be made once
 * (the reference builds its weight tensors once in the plugin constructor,
 * modulatedDeformableConv2dPlugin.cpp:33-71).  F32 / F16 / I8 (I8: rows zero-padded to 16 bytes, for
 * bevops_mdconv_forward_int8_packed); `packed` holds bevops_mdconv_packed_weight_size bytes, 16-byte aligned. */
size_t bevops_mdconv_packed_weight_size(int dtype, int Cout, int Cin_per_group, int Kh, int Kw);
int bevops_mdconv_pack_weight(int dtype, const void *weight, void *packed, int Cout,
                              int Cin_per_group, int Kh, int Kw, void *stream);
/* Channels-last variant for a caller whose activations are [B, H, W, C] (the re-hosted backbone):
 * input and output NHWC, packed weights, optional fused ReLU; fp16 fused-kernel domain only
 * (NOT_SUPPORTED otherwise).  offset_mask_channels == 0: offset / mask keep the reference's
 * planar [B, ., Ho, Wo] layout.  offset_mask_channels == OC > 0: `offset` is the raw channels-last
 * output [B, Ho, Wo, OC] of the pack's offset convolution (cnn/dcn.py:62-70) for ONE deform group:
 * 2*KK offset channels (h, w per tap) then KK mask logits, OC >= 3*KK and even (BAD_PARAM otherwise),
 * channels >= 3*KK ignored; `mask` is ignored and the sigmoid is applied in the kernel.
 * deform_groups > 1 with offset_mask_channels > 0 is NOT_SUPPORTED (a pack with several deform groups
 * orders its channels differently); planar offsets take any deform_groups of the fused domain. */
int bevops_mdconv_forward_nhwc(int dtype, const void *input_nhwc, const void *offset,
                               const void *mask, const void *packed_weight, const void *bias,
                               void *output_nhwc, int relu, int offset_mask_channels,
                               void *workspace, size_t workspace_bytes,
                               int B, int Cin, int H, int W, int Cout, int Kh, int Kw, int stride_h,
                               int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int groups,
                               int deform_groups, void *stream);
/* x[rows, channels] += bias[channels] (+ residual[rows, channels]), optional ReLU, in place: the
 * folded-BN convolution epilogue of the re-hosted backbone as one pass (fp16, channels % 8 == 0). */
int bevops_bias_act_nhwc(int dtype, void *x, const void *bias, const void *residual, size_t rows,
                         int channels, int relu, void *stream);
/* Stem epilogue of the channels-last backbone in one pass: out [N, Ho, Wo, C] = max_pool2d(relu(x + bias), 3,
 * stride 2, pad 1) over the convolution's raw output x [N, H, W, C] (fp16, C % 8 == 0; Ho = (H - 1) / 2 + 1).
 * Bit-equal to bevops_bias_act_nhwc followed by the framework's max_pool2d (rounding is monotonic). */
int bevops_bias_relu_maxpool_nhwc(int dtype, const void *x, const void *bias, void *out, int n, int h, int w,
                                  int channels, void *stream);
/* The whole ResNet stem of the re-hosted backbone as ONE kernel (round 5; not a reference plugin): conv 7x7 / stride 2 /
 * pad 3 from 3 to 64 channels (folded-BN shift `bias`) -> ReLU -> max_pool2d 3 / stride 2 / pad 1
 * (third_party/bev_mmdet3d/models/backbones/resnet.py:619-624: conv1, norm1, relu, maxpool), from the PLANAR camera
 * images x [n, 3, h, w] (fp16, w even) to the pooled channels-last activation out [n, hp, wp, 64]
 * (hc = (h - 1) / 2 + 1, hp = (hc - 1) / 2 + 1, likewise w), fp16 or -- out_dtype BEVOPS_I8, scale_out -- int8 with
 * q = min(rne(v / scale_out), 127): the first tensor of the INT8 engine's activation chain.  fp32 accumulation, one
 * rounding at the end (the two-pass form rounds the convolution's output to fp16 first: results agree to that
 * rounding).  bevops_stem_pack turns weight [64, 3, 7, 7] + bias [64] (fp16; bias may be NULL) into the kernel's
 * matrix-core operand image (bevops_stem_packed_size bytes, 16-byte aligned, device memory): once per model.
 * bevops_stem_set_variant (thread-local, A/B switch of the tests): 0 = pooling neighbours through wave-wide DPP
 * shifts, 1 = through ds_bpermute; identical results.  Returns the previous value. */
size_t bevops_stem_packed_size(void);
int bevops_stem_pack(int dtype, const void *weight, const void *bias, void *packed, void *stream);
int bevops_stem_conv_pool(int dtype, int out_dtype, const void *x, const void *packed, void *out, int n, int h, int w,
                          float scale_out, void *stream);
int bevops_stem_set_variant(int variant);

/* FPN top-down step of the re-hosted neck on channels-last fp16 activations (not a reference plugin):
 * a[n, y, x, :] += b[n, sy(y), sx(x), :], source indices as aten's nearest up-sampling -- the reference's
 * `laterals[i-1] += F.interpolate(laterals[i], size=..., mode="nearest")`
 * (third_party/bev_mmdet3d/models/necks/fpn.py:170-176) in one pass, bit-equal to it.  In place on `a`. */
int bevops_upsample_add_nhwc(int dtype, void *a, const void *b, int n, int h, int w, int hb, int wb,
                             int channels, void *stream);

/* BEVDet's view transformer between depth_net and the pooling (not a reference plugin;
 * det2trt/models/detector/bevdet.py:50-76: softmax over the depth bins, the feature slice, their layout copies) as ONE
 * launch.  x: [n * hw, row_stride] fp16, channels-last pixel rows with the depth logits in columns
 * depth_offset .. depth_offset + D and the features in feat_offset .. feat_offset + C.  depth: [n, D, hw] fp16 (the
 * [N, D, H, W] tensor bev_pool_v2 indexes by ranks_depth) = the softmax over each pixel's D logits: maximum subtracted,
 * exponentials and their sum in fp32, one division, one rounding.  feat: [n, hw, C] fp16, the feature columns bit for
 * bit.  Domain: BEVOPS_F16 and 1 <= D <= 256 (else NOT_SUPPORTED); C > 0, C % 8 == 0, feat_offset % 8 == 0,
 * row_stride % 8 == 0, both column ranges inside the row and disjoint, x and feat 16-byte aligned (else BAD_PARAM).
 * n * hw == 0: success, no launch.  No allocation, no synchronisation; capturable. */
int bevops_lss_depth_split(int dtype, const void *x, void *depth, void *feat, int n, int hw, int row_stride,
                           int depth_offset, int D, int feat_offset, int C, void *stream);

/* FPN_LSS's `cat([a, interpolate(b, mode="bilinear", align_corners=True)], 1)` (models/necks/lss_fpn.py) on
 * channels-last fp16 activations in one pass (not a reference plugin): out [n, h, w, ca + cb]; a [n, h, w, ca] is
 * copied into the first ca channels (a == NULL with ca == 0: the plain up-sampling); b [n, hb, wb, cb].  Output row y
 * reads source row y * (hb - 1) / (h - 1) (0 when h == 1), columns likewise, evaluated as an exact fraction: the
 * first / last outputs are the first / last inputs and an equal-size axis is the identity.  Four corners weighted in
 * fp32, one rounding.  Any h, w, hb, wb >= 1.  ca % 8, cb % 8, 16-byte alignment, a == NULL with ca > 0: BAD_PARAM;
 * a dtype other than BEVOPS_F16: NOT_SUPPORTED. */
int bevops_upsample_bilinear_concat_nhwc(int dtype, const void *a, const void *b, void *out, int n, int h, int w,
                                         int ca, int hb, int wb, int cb, void *stream);

/* bevops_lss_depth_split's INT8 sibling (csrc/lss_split_s8.hip; the BEV half of the INT8 build of BEVDet): the fp16
 * rows [n * hw, row_stride] depth_net wrote -> depth_q int8 [n, D, hw] (plane-major) and feat_q int8 [n, hw, C], exactly
 * the operands bevops_bev_pool_v2_forward takes in BEVOPS_I8.  Every step ONE fp32 operation in exactly this order
 * (inv_d = 1.f / scale_depth and inv_f = 1.f / scale_feat are computed once on the host in fp32):
 *   m      = maximum of the pixel's D logits                          (exact)
 *   e_d    = expf(x_d - m)
 *   sum    : four lanes per pixel; lane j adds its bins j, j + 4, j + 8, ... in ascending order to 0.f, then
 *            s = s + s[lane ^ 1]; s = s + s[lane ^ 2], i.e. (s0 + s1) + (s2 + s3) of the four lane sums
 *   p      = e_d / sum                                                (IEEE division; the build has no fast-math)
 *   q      = min(max(rne(p * inv_d), -127), 127)
 *   feat_q = min(max(rne((float)x * inv_f), -127), 127)
 * A NaN leaves as -127 (as in bevops_conv_slice_s8's epilogue).  A non-finite logit spoils its own pixel's D bytes and
 * nothing else.  Domain: 1 <= D <= 256 (else NOT_SUPPORTED); C > 0, C % 16 == 0, feat_offset % 8 == 0,
 * row_stride % 8 == 0, both column ranges inside the row and disjoint, x_f16 and feat_q 16-byte aligned (depth_q any
 * address: a plane leaves as whole dwords where its address allows, as bytes otherwise), both scales positive and
 * finite (else BAD_PARAM; NULL pointers, n < 0, hw < 0 too).  n == 0 or hw == 0: SUCCESS without a launch.  One launch,
 * no atomics, no scratch, no allocation, no synchronisation; capturable. */
int bevops_lss_depth_split_s8(const void *x_f16, void *depth_q, void *feat_q, int n, int hw, int row_stride,
                              int depth_offset, int D, int feat_offset, int C, float scale_depth, float scale_feat,
                              void *stream);

/* out[n, y, x, 0 .. C) = F.interpolate(b, (h, w), mode="bilinear", align_corners=True) on the INT8 channel slice b,
 * requantised (csrc/lss_split_s8.hip).  b_q [n, hb, wb] pixels and out_q [n, h, w] pixels point at the first channel of
 * a slice; pitches in elements, as in bevops_conv_slice_s8 and bevops_upsample_nearest2x_nhwc.  FPN_LSS's concatenation
 * disappears: the producer of the other channels writes its slice of the consumer's buffer itself, this entry writes
 * the rest; there is no `a` operand and no copy.  The source position is bevops_upsample_bilinear_concat_nhwc's exact
 * fraction.  On the four corners converted exactly to fp32, in this order, with r = scale_b * (1.f / scale_out)
 * computed on the host in fp32:
 *   hx = 1 - lx, hy = 1 - ly
 *   t = hx * v00;  t = fma(lx, v01, t);  u = hx * v10;  u = fma(lx, v11, u);  o = hy * t;  o = fma(ly, u, o);  v = o * r
 *   q = min(max(rne(v), -127), 127)
 * Domain: C > 0 and C % 16 == 0, pitches multiples of 16 and at least C, slices on 16-byte boundaries, b not overlapping
 * out (disjoint channel slices of one buffer with equal pitches are accepted), n >= 0, h, w, hb, wb >= 1, scales
 * positive and finite (else BAD_PARAM); h * hb or w * wb of 2^31 or more, n hb wb or n h w of 2^31 or more:
 * NOT_SUPPORTED.  n == 0: SUCCESS without a launch. */
int bevops_upsample_bilinear_s8(const void *b_q, int b_pitch, float scale_b, void *out_q, int out_pitch, float scale_out,
                                int n, int h, int w, int hb, int wb, int C, void *stream);

/* Encoder input assembly (det2trt/models/modules/transformer.py:138-152): dst[n, r, :] = (src[n, r, :] +
 * cam_embed[n, :]) + level_embed[:], both sums rounded to fp16 like the two tensor adds they replace; `dst` is
 * the level's first row inside the concatenated [cams, sum hw, C] feature tensor, `dst_batch_stride` its
 * element stride between cameras (so no torch.cat copy is needed).  src: [n, rows, C] dense. */
int bevops_feat_embed_nhwc(int dtype, const void *src, const void *cam_embed, const void *level_embed, void *dst,
                           int n, size_t rows, int channels, size_t dst_batch_stride, void *stream);
/* The DCNv2 pack's offset convolution (cnn/dcn.py:62-70: 3x3, stride 1, pad 1, Cout <= 32) on
 * channels-last fp16 activations with its bias in the epilogue:
 *   output_nhwc[B, H, W, 32] = conv3x3(input_nhwc[B, H, W, Cin], weight[Cout, Cin, 3, 3]) + bias32
 * (channels >= Cout are the bias32 values, normally 0).  Cin in {64, 128, 256} or a multiple of
 * 256.  The weight is packed once (bevops_conv3x3_c32_pack_weight into a caller buffer of
 * bevops_conv3x3_c32_packed_weight_size bytes; 0 = unsupported Cin); bias32 has 32 entries or is
 * NULL.  The result is the `offset` operand of bevops_mdconv_forward_nhwc with
 * offset_mask_channels = 32. */
size_t bevops_conv3x3_c32_packed_weight_size(int dtype, int Cin);
int bevops_conv3x3_c32_pack_weight(int dtype, const void *weight, void *packed, int Cout, int Cin, void *stream);
/* 0 = default: at Cin == 256 the build with the weights in registers and 8 x 8-pixel image tiles in LDS (round 6),
 * the tile kernel with three waves per 32-pixel tile otherwise; 3 = that tile kernel everywhere (round 5's default;
 * bit-identical to 0); 2 = the tile kernel with one wave per tile (rounds 1-4); 1 = the variant that stages the
 * image rows in LDS (A/B, tests).  Returns the previous value. */
int bevops_conv3x3_c32_set_variant(int variant);
int bevops_conv3x3_c32_forward_nhwc(int dtype, const void *input_nhwc, const void *packed_weight,
                                    const void *bias32, void *output_nhwc, int B, int H, int W, int Cin,
                                    void *stream);
/* A/B switch of bevops_rotate_forward's store path (thread-local): 0 = 16-byte stores through an LDS transpose of
 * 8-pixel runs where every plane starts 16-byte aligned, 1 = one store per lane and plane (rounds 1-3).  Same values
 * either way.  Returns the previous setting. */
int bevops_rotate_set_variant(int variant);
/* Temporal self-attention glue (round 5; not reference plugins; modules/temporal_self_attention.py:350-457).
 * bevops_tsa_split: one row of the stacked sampling_offsets | attention_weights projection, laid out as the reference
 * views it -- [heads][bev_queue 2][points][xy] then [heads][bev_queue 2][points] -- split into the queue-major operands
 * of the MSDA call: offsets [2, num_query, heads, points * 2], weights [2, num_query, heads, points] (what
 * .view(...).permute(0, 3, 1, 2, 4, 5[, 6]).contiguous() produces twice, as one pass).  fp16, points == 4.
 * bevops_queue_mean2: out[i] = (x[i] + x[count + i]) / 2 in fp32 with one rounding (= torch.mean over the two queue
 * entries), fp16, count % 8 == 0. */
int bevops_tsa_split(int dtype, const void *both, void *offsets, void *weights, int num_query, int heads, int points,
                     void *stream);
int bevops_queue_mean2(int dtype, const void *x, void *out, size_t count, void *stream);
/* bevops_rotate_forward on channels-last data: img / output are [height, width, channels] (fp32 /
 * fp16, channels a multiple of 4 / 8) -- the layout prev_bev [H*W, 1, C] already has in the model,
 * so the permute-copy to [C, H, W] and back around the plugin (transformer.py:296-303) disappears.
 * Same arithmetic, element for element. */
int bevops_rotate_forward_hwc(int dtype, const void *img, const void *angle, const void *center,
                              int angle_dtype, void *output, int channels, int height, int width,
                              int interpolation, void *stream);
/* out[rows, channels] = (x - mean) * rsqrt(var + eps) * gamma + beta over the last dimension
 * (biased variance, fp32 statistics; torch.nn.LayerNorm semantics); fp16, channels in
 * {64, 128, 256, 512}; gamma / beta optional; out may alias x.  The norms between the attention
 * blocks of the re-hosted encoder / decoder (encoder.py:510-636) as one streaming pass. */
int bevops_layer_norm(int dtype, const void *x, const void *gamma, const void *beta, void *out,
                      size_t rows, int channels, float eps, void *stream);
/* INT8 dense layers: what TensorRT builds from the reference's `LinearQ` /
 * `Conv2dQ` (= pytorch_quantization QuantLinear / QuantConv2d, det2trt/models/utils/register.py:78-84):
 * per-tensor symmetric quantisation of the layer input, int8 x int8 -> int32 GEMM on the matrix cores,
 * de-quantising epilogue.  Not plugins.
 *   bevops_quantize_rows: q = clamp(rne(x / scale), -127, 127), x fp16, count % 8 == 0.
 *   bevops_linear_int8:   out[M, N] = act((a_q[M, K] . w_q[N, K]^T) * scale_a * w_scale[n] + bias[n]
 *                         + residual[M, N]); w_scales (device, fp32 [N]) per output channel, or NULL
 *                         for the per-tensor scale_w; bias fp32 (device) optional; residual fp16
 *                         optional; out fp16, or int8 requantised with scale_out.  K % 16 == 0.
 *   bevops_linear_int8_fused: the same layer taking the fp16 activation x[M, K] itself: it is quantised
 *                         inside the GEMM's operand load, q = clamp(rne(x * (1 / scale_a)), -127, 127) with
 *                         the product and the rounding in one fused multiply-add -- no quantise pass, no int8
 *                         copy of the activation.  (x * fl(1 / s) against fl(x / s): the two quantisers can
 *                         differ by one step only where x / s is within 1e-5 of a rounding tie.)
 *   bevops_dequantize_rows: out (fp16) = q (int8) * scale, product in fp32, one rounding; count % 8 == 0. */
int bevops_quantize_rows(int dtype, const void *x, void *q, size_t count, float scale, void *stream);
int bevops_dequantize_rows(int dtype, const void *q, void *out, size_t count, float scale, void *stream);
int bevops_linear_int8(const void *a_q, float scale_a, const void *w_q, const float *w_scales,
                       float scale_w, const float *bias, const void *residual, int out_dtype,
                       void *out, float scale_out, long long M, int N, int K, int relu, void *stream);
int bevops_linear_int8_fused(const void *x_f16, float scale_a, const void *w_q, const float *w_scales,
                             float scale_w, const float *bias, const void *residual, int out_dtype,
                             void *out, float scale_out, long long M, int N, int K, int relu, void *stream);
/* The same tiled GEMM skeleton (csrc/tile_gemm.hip) with fp16 operands: out[M, N] = act(x[M, K] . w[N, K]^T +
 * bias[n] + residual[M, N]), fp32 accumulation, one rounding; bias / residual fp16, optional.  K % 8 == 0.
 * One of the implementations the host layer's measured dispatch (functions/linear.py: dense_auto) picks from,
 * next to bevops_tsgemm_f16 and bevops_linear_bias_act. */
int bevops_tile_gemm_f16(const void *x, const void *weight, const void *bias, const void *residual,
                         void *out, long long M, int N, int K, int relu, void *stream);
/* One GEMM over TWO activation sources (the first bottleneck of a ResNet stage: conv3 and the downsample convolution
 * as one accumulation, no identity tensor written and read back):
 *     out[m, n] = act( sum_{k < K1} a1[m, k] w[n, k] + sum_{k < K2} a2row(m)[k] w[n, K1 + k] + bias[n] )
 * a1 [M, K1] fp16 rows; a2 a channels-last [a2_B, a2_H, a2_W, K2] fp16 tensor whose row m is pixel
 * (b, a2_stride * ho, a2_stride * wo) with m = (b * Ho + ho) * Wo + wo, Ho = (a2_H - 1) / a2_stride + 1 (Wo alike): the
 * row addressing of bevops_conv_tile_f16 with ksize 1 (a2_stride 1: a plain [M, K2] matrix); weight [N, K1 + K2] the
 * two layers' weights side by side, bias fp16 [N] (their sum) or NULL; out [M, N] fp16.  k runs over source 1 ascending,
 * then source 2 ascending, in fp32, ONE rounding: bit for bit the single-source entry of the same kernel family on the
 * materialised [a1 | rows of a2] -- bevops_tsgemm_f16 (weight-stationary kernel) for K1 + K2 <= 256 and N % 256 == 0,
 * bevops_tile_gemm_f16 otherwise.  An output row depends on its own operands only.  No workspace.
 * K1 or K2 no positive multiple of 64, N % 8 != 0, a2_stride outside {1, 2}, a byte range of a1 / a2 / weight from
 * 0xFFFFFF00 on: BEVOPS_NOT_SUPPORTED.  NULL a1 / a2 / weight / out, non-positive sizes, M != a2_B * Ho * Wo, pointers
 * not 16-byte aligned: BEVOPS_BAD_PARAM.  Nothing is queued unless BEVOPS_SUCCESS is returned. */
int bevops_gemm2_f16(const void *a1, const void *a2, const void *weight, const void *bias, void *out, long long M, int N,
                     int K1, int K2, int a2_B, int a2_H, int a2_W, int a2_stride, int relu, void *stream);
/* Several layers that read the SAME rows as one launch of that kernel: weight [N, K] / bias [N] are the layers'
 * parameters stacked, and a table of at most 8 destinations says where each column range of the product goes --
 * columns [col_begin, col_end) as a pitched fp16 matrix of their own (element (m, col_begin + c) at
 * out[m * out_pitch + c]) with identity rows of their own (res[m * res_pitch + c], or NULL).  Exactly the bytes of
 * the separate bevops_tile_gemm_f16 launches on weight[col_begin:col_end]; columns outside every range and the bytes
 * between pitched rows are never written.  Range bounds are multiples of 64, ranges do not overlap, pitches are
 * multiples of 8 elements and at least the range's width, pointers 16-byte aligned (else BEVOPS_BAD_PARAM); N > 64. */
typedef struct bevops_gemm_dst {
  int col_begin, col_end;
  void *out;
  long long out_pitch;
  const void *res;
  long long res_pitch;
} bevops_gemm_dst;
int bevops_tile_gemm_f16_dst(const void *x, const void *weight, const void *bias, const bevops_gemm_dst *dst, int num_dst,
                             long long M, int N, int K, int relu, void *stream);
/* The same table on the few-row GEMM (bevops_small_gemm_f16: 32 x 64 tiles, K % 64 == 0, K <= 1024, M <= 65536) -- the
 * decoder's sampling_offsets | attention_weights over the same 900 queries (N = 64 + 32, the two cached query_pos terms as
 * identities) as one launch.  Here a range begins on a multiple of 64 and ends on a multiple of 8, and no two ranges share
 * a 64-column block.  Exactly the bytes of the separate bevops_small_gemm_f16 launches. */
int bevops_small_gemm_f16_dst(const void *x, const void *weight, const void *bias, const bevops_gemm_dst *dst, int num_dst,
                              long long M, int N, int K, int relu, void *stream);
/* A CHAIN of up to 8 dense stages over the same M rows as ONE launch (the decoder's 900 object queries: the rows of
 * the intermediate stages never leave the chip; csrc/row_chain.hip, design/model.md "Row chains"):
 *     y_s = act( LayerNorm( in_s @ weight_s.T + bias_s + identity_s ) ),  fp16 operands, fp32 sums, ONE rounding per stage.
 * in_s is the output of stage `input` (-1: the stage in front; for stage 0: x [M, K_0], row pitch x_pitch).  identity_s
 * is `res` (rows of pitch res_pitch) or, with res_stage = r <= s, the INPUT rows of stage r, or absent.  `norm` != 0:
 * LayerNorm over the N columns (gamma, beta [N], eps; mean and centred squares in fp32 over the unrounded row) in front
 * of `act` (0 none, 1 ReLU).  Columns [col_begin, col_end) of the stage go to dst[i].out (pitched, num_dst <= 2,
 * col_begin % 8 == 0, ranges ascending); a stage with num_dst == 0 stores nothing.  A row's results depend on that
 * row's operands only.  packed != 0: `weight` is in the order the matrix instruction reads it -- element (n, k) of the
 * [N, K] matrix at ((((n / 16) * (K / 32) + k / 32) * 64 + n % 16 + 16 * ((k % 32) / 8)) * 8 + k % 8, N rounded up to whole
 * 16-row tiles with zero rows -- so that a wave's request is one contiguous kilobyte; the bits are those of the
 * row-major call.  groups = G > 1: every row operand holds G * M rows and weight / bias / gamma / beta are stacked
 * [G, N, K] / [G, N]; rows g * M .. (g + 1) * M - 1 use group g.
 * Domain: K % 32 == 0, K <= 768, N <= 768, at most 8 stages, 16-byte aligned pointers, x_pitch % 8 == 0, a tensor
 * identity with N % 4 == 0 and res_pitch % 4 == 0, row operands below 0xFFFFFF00 bytes, the stages' row tiles
 * within 160 KB of LDS -- else BEVOPS_NOT_SUPPORTED.  NULL / inconsistent arguments (a stage's K against its input's
 * width, an identity's width against N, ranges outside N): BEVOPS_BAD_PARAM.  Nothing is queued unless BEVOPS_SUCCESS. */
typedef struct bevops_chain_dst {
  int col_begin, col_end;
  void *out;
  long long pitch;
} bevops_chain_dst;
typedef struct bevops_chain_stage {
  const void *weight, *bias;
  int K, N;
  int input, act;
  int packed;
  const void *res;
  long long res_pitch;
  int res_stage, norm;
  const void *gamma, *beta;
  float eps;
  int num_dst;
  bevops_chain_dst dst[2];
} bevops_chain_stage;
int bevops_row_chain_f16(const void *x, long long x_pitch, const bevops_chain_stage *stages, int num_stages, long long M,
                         int groups, void *stream);
/* Convolution on channels-last fp16 activations as an implicit GEMM on the same tiled skeleton (no column
 * buffer, no strided copy): kernel ksize x ksize in {1, 3}, pad ksize / 2, any stride.  x [B, H, W, Cin],
 * weight_taps [Cout][ksize][ksize][Cin] (= weight.permute(0, 2, 3, 1)), out [B, Hout, Wout, Cout] =
 * act(conv(x) + bias[n] + residual); bias / residual fp16, optional.  Cin % 32 == 0.  The plain 3x3
 * convolutions of the re-hosted backbone / neck (ResNet stages without DCN: resnet.py:106-260; FPN output
 * and extra convolutions: necks/fpn.py:140-155) and the stride-2 1x1 convolutions at the head of a stage,
 * with their shift and ReLU in the epilogue. */
int bevops_conv_tile_f16(const void *x, const void *weight_taps, const void *bias, const void *residual,
                         void *out, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int relu,
                         void *stream);
/* The 3x3 / stride 1 / pad 1 convolution of a 64-channel layer (conv2 of the ResNet stage-1 bottlenecks,
 * det2trt/models/backbones/resnet.py:106-260) with BOTH operands in LDS: the 64 x 576 weight matrix resident per
 * persistent block, 16 x 16-pixel output tiles whose 18 x 18 input pixels are staged once (a tap is an LDS address
 * offset).  Same operands and layouts as bevops_conv_tile_f16 (no identity rows); results bit-identical to it.
 * NOT_SUPPORTED unless Cin == Cout == 64. */
int bevops_conv3x3_c64_f16(const void *x, const void *weight_taps, const void *bias, void *out, int B, int H, int W,
                           int Cin, int Cout, int relu, void *stream);
/* ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1) + bias + ReLU on channels-last fp16 activations (the up-sampling
 * layers of mmdet's CTResNetNeck; csrc/deconv.hip) as four implicit GEMMs on the same tiled skeleton, one per output
 * parity: no column buffer, no zero-stuffed input.  x [B, H, W, Cin], out [B, 2H, 2W, Cout] =
 * act(conv_transpose2d(x, weight, stride 2, padding 1) + bias[co]); fp32 accumulation, bias / ReLU in fp32, one
 * rounding; bias fp16, optional.  `packed_weight` is the layer's [Cin, Cout, 4, 4] weight (PyTorch's layout) in the
 * order [parity 2 py + px][Cout][dy][dx][Cin], element = weight[ci][co][3 - py - 2 dy][3 - px - 2 dx]:
 * bevops_deconv4x4s2_pack_weight writes it (once per weight tensor; bevops_deconv4x4s2_packed_weight_size bytes, 0 for
 * a layer outside the domain).  fp16 only, Cin % 32 == 0 (a k-step never straddles two taps), Cout % 8 == 0, any
 * other dtype / ksize / stride / pad: BEVOPS_NOT_SUPPORTED.  Non-positive dimensions, NULL operands, x / packed_weight /
 * out not 16-byte aligned: BEVOPS_BAD_PARAM.  B == 0: nothing launched, BEVOPS_SUCCESS.  x and the packed weight are
 * addressed through 32-bit byte offsets: each must be smaller than 0xFFFFFF00 bytes (B H W Cin < 2 147 483 520
 * elements), else BEVOPS_NOT_SUPPORTED; the output is addressed through 64-bit pointers. */
size_t bevops_deconv4x4s2_packed_weight_size(int dtype, int Cin, int Cout);
int bevops_deconv4x4s2_pack_weight(int dtype, const void *weight, void *packed, int Cin, int Cout, void *stream);
int bevops_deconv4x4s2_f16(int dtype, const void *x, const void *packed_weight, const void *bias, void *out, int B, int H,
                           int W, int Cin, int Cout, int ksize, int stride, int pad, int relu, void *stream);
/* Convolution on CHANNEL SLICES of channels-last fp16 tensors with the activation in the epilogue (csrc/conv_slice.hip;
 * the convolutions of YOLOX's CSPDarknet, PAFPN and head): the same tiled implicit GEMM as bevops_conv_tile_f16, but
 * x, residual and out each point at the first channel of a slice of a wider channels-last tensor -- element
 * (b, y, x, c) lives at base + ((b H + y) W + x) pitch + c, every pitch in elements, at least the slice's channel count
 * and a multiple of 8 -- so a layer reads one operand of a concatenation and writes its share of the next one.
 *   out = act(conv(x) + bias[co]) + residual     kernel ksize in {1, 3}, pad ksize / 2, stride in {1, 2}
 * The identity is added AFTER the activation (mmdet's DarknetBottleneck).  act: 0 none, 1 ReLU, 2 SiLU = v * sigmoid(v)
 * in fp32 (hardware exponential and reciprocal).  fp32 accumulation, bias / activation / identity in fp32, ONE rounding.
 * weight_taps [Cout][ksize][ksize][Cin] as for bevops_conv_tile_f16; bias fp16 [Cout], optional; residual optional;
 * out [B, Hout, Wout] pixels of Cout channels.  x and out MAY be disjoint channel slices of one buffer (every access
 * is a 16-byte vector inside its own slice); out and residual may be the same slice; x must not overlap out.
 * Cin % 32 == 0, Cout % 8 == 0, ksize / stride / act outside the lists: BEVOPS_NOT_SUPPORTED.  NULL x / weight_taps /
 * out, non-positive sizes, a pitch below the channel count or no multiple of 8, x / weight_taps / residual / out not
 * 16-byte aligned: BEVOPS_BAD_PARAM.  x and the weight are addressed through 32-bit byte offsets: B H W x_pitch and
 * Cout ksize^2 Cin must stay below 0xFFFFFF00 bytes, else BEVOPS_NOT_SUPPORTED.  B == 0: nothing launched,
 * BEVOPS_SUCCESS.  With pitch == channels, no residual and act in {0, 1} the result equals bevops_conv_tile_f16's bit
 * for bit. */
int bevops_conv_slice_f16(const void *x, int x_pitch, const void *weight_taps, const void *bias, const void *residual,
                          int res_pitch, void *out, int out_pitch, int B, int H, int W, int Cin, int Cout, int ksize,
                          int stride, int act, void *stream);
/* bevops_conv_slice_f16 with a DILATION and an optional PER-IMAGE bias (the ASPP block of BEVDepth's DepthNet;
 * csrc/conv_slice.hip, the same kernels: both are block-uniform runtime values).  bevops_conv_slice_f16 forwards here
 * with (dilation, bias_pitch) = (1, 0) and keeps its bits.
 *   dilation >= 1, pad = dilation * (ksize / 2): tap (ky, kx) of output pixel (y, x) reads input pixel
 *     (y + (ky - 1) dilation, x + (kx - 1) dilation), zero outside the image; stride 1 keeps the size.
 *   bias_pitch == 0: the shared bias[co].  bias_pitch != 0: bias is fp16 [B][bias_pitch] and output row m = pixel
 *     (b, y, x) takes bias[b * bias_pitch + co] -- the image of every ROW, a row tile may hold several images.
 * Statuses, in this order: everything BEVOPS_BAD_PARAM of bevops_conv_slice_f16, and dilation <= 0; bias_pitch != 0
 * with a NULL bias, bias_pitch < Cout, bias_pitch % 8 != 0 or a bias not 16-byte aligned: BEVOPS_BAD_PARAM.  Then
 * everything BEVOPS_NOT_SUPPORTED of bevops_conv_slice_f16; dilation > 1 with ksize != 3 or stride != 1:
 * BEVOPS_NOT_SUPPORTED.  32-bit byte offsets: B H W x_pitch and Cout ksize^2 Cin below 0xFFFFFF00 bytes as there (a tap
 * inside the image lies inside that extent), and with dilation > 1 the displacement of a tap, computed for taps
 * outside the image too, must fit a signed 32-bit byte count: dilation (W + 1) x_pitch 2 <= 0x7FFFFFFF, else
 * BEVOPS_NOT_SUPPORTED.  B == 0: BEVOPS_SUCCESS without a launch. */
int bevops_conv_slice_f16_ex(const void *x, int x_pitch, const void *weight_taps, const void *bias, const void *residual,
                             int res_pitch, void *out, int out_pitch, int B, int H, int W, int Cin, int Cout, int ksize,
                             int stride, int act, int dilation, int bias_pitch, void *stream);
/* The layers of BEVDepth's DepthNet that are no convolution (csrc/lss_depthnet.hip; LSSViewTransformerBEVDepth,
 * bevformer_tensorrt_amd/bevdepth.py).  None allocates, synchronises or uses atomics; n == 0: BEVOPS_SUCCESS without a
 * launch.
 *
 * bevops_lss_camera_gate: the camera-aware squeeze-excite gates.  mlp_input fp32, camera i's 27 calibration values at
 *   mlp_input + i * in_pitch (in_pitch >= 27, in floats); gates fp32 [2][n][mid], branch 0 = depth, 1 = context:
 *     gates[br][i][:] = sigmoid(expand(relu(reduce(fc2(relu(fc1(bn(v_i))))))))
 *   All arithmetic fp32.  Every layer: acc = 0; for k = 0, 1, ...: acc = fma(w[k][j], in[k], acc); y[j] = acc + b[j]
 *   (ONE fused multiply-add per term, ascending k, the bias added last with one rounding); relu = max(y, 0);
 *   sigmoid(y) = 1 / (1 + exp(-y)) with expf and an IEEE division.
 *   packed: one fp32 block of bevops_lss_camera_gate_packed_size(mid) bytes (0 outside the domain), branch 0 then
 *   branch 1, each branch
 *     W1 [27][mid]   b1 [mid]     fc1 with the frozen BatchNorm1d(27) folded in: W1[k][j] = fc1.w[j][k] s[k],
 *                                 b1[j] = fc1.b[j] + sum_k fc1.w[j][k] t[k], s = gamma / sqrt(var + eps), t = beta - mean s
 *     W2 [mid][mid]  b2 [mid]     fc2,         W2[k][j] = fc2.w[j][k]        (every matrix K-MAJOR: [input k][output j])
 *     Wr [mid][mid]  br [mid]     conv_reduce, Wr[k][j] = conv_reduce.w[j][k]
 *     We [mid][mid]  be [mid]     conv_expand, We[k][j] = conv_expand.w[j][k]
 *   = mid (3 mid + 31) words per branch.  One block per (camera, branch).
 *   Statuses, in this order: NULL mlp_input / packed / gates, n < 0, mid <= 0, in_pitch < 27, a pointer not 4-byte
 *   aligned: BEVOPS_BAD_PARAM; mid % 8 != 0, mid < 8, mid > 512, n > 0x3FFFFFFF: BEVOPS_NOT_SUPPORTED.
 * bevops_se_gate2_nhwc: x fp16, n images of hw pixels of c channels (pixel p of image i at x + (i hw + p) x_pitch);
 *     out_a[i, p, ch] = fp16(float(x[i, p, ch]) * gates[0][i][ch])      out_b: the same with gates[1]
 *   gates fp32 [2][n][c] as bevops_lss_camera_gate writes them (mid == c).  One fp32 product, one rounding; x is read
 *   once; 16-byte vectors.  x, out_a, out_b are channel slices as in bevops_conv_slice_f16 (pitches in elements, >= c,
 *   multiples of 8); out_a / out_b must not overlap x or each other.
 *   Statuses, in this order: NULL operands, n < 0, hw <= 0, c <= 0, a pitch below c or no multiple of 8, x / gates /
 *   out_a / out_b not 16-byte aligned: BEVOPS_BAD_PARAM; c % 8 != 0, more than 2^31 - 1 blocks of 256 vectors:
 *   BEVOPS_NOT_SUPPORTED.
 * bevops_global_avgpool_nhwc: out[i, ch] = fp16((sum_p float(x[i, p, ch])) / float(hw)), out fp16 [n][out_pitch].
 *   The fp32 sum has a FIXED order that depends on (hw, c) alone: s_l = x[l] + x[l + 32] + x[l + 64] + ... (ascending,
 *   from 0.f) for l = 0 .. 31, total = (((s_0 + s_1) + s_2) + ... ) + s_31; then one IEEE division and one rounding.  Two
 *   calls give equal bits.
 *   Statuses, in this order: NULL operands, n < 0, hw <= 0, c <= 0, x_pitch below c or no multiple of 8, out_pitch < c,
 *   x not 16-byte aligned, out not 2-byte aligned: BEVOPS_BAD_PARAM; c % 8 != 0, n ceil(c / 64) > 2^31 - 1:
 *   BEVOPS_NOT_SUPPORTED. */
size_t bevops_lss_camera_gate_packed_size(int mid);
int bevops_lss_camera_gate(const float *mlp_input, int in_pitch, const void *packed, float *gates, int n, int mid,
                           void *stream);
int bevops_se_gate2_nhwc(const void *x, int x_pitch, const float *gates, void *out_a, int a_pitch, void *out_b,
                         int b_pitch, int n, int hw, int c, void *stream);
int bevops_global_avgpool_nhwc(const void *x, int x_pitch, void *out, int out_pitch, int n, int hw, int c, void *stream);
/* The data-movement layers of YOLOX on the same channel slices (csrc/yolox.hip); fp16, exact, 16-byte vectors of 8
 * channels.  Statuses as bevops_conv_slice_f16: NULL / unaligned operands, non-positive sizes, bad pitches:
 * BEVOPS_BAD_PARAM; C % 8 != 0, odd H or W (focus), a pool size that is even or above 13, a buffer of 0xFFFFFF00 bytes
 * or more: BEVOPS_NOT_SUPPORTED; B == 0: BEVOPS_SUCCESS without a launch.
 * bevops_focus_nhwc: mmdet's Focus.  image planar [B, 3, H, W] -> out [B, H/2, W/2] pixels of 32 channels: channel
 *   3 p + c = image[b, c, 2 y + (p & 1), 2 x + (p >> 1)] for p = 0 .. 3 (top-left, bottom-left, top-right, bottom-right),
 *   channels 12 .. 31 = 0 (the stem convolution then is a bevops_conv_slice_f16 with Cin = 32 and zero weight columns).
 * bevops_spp_maxpool_nhwc: SPPBottleneck's three stride-1 "same" max-pools (odd sizes k0, k1, k2 <= 13, padding -inf)
 *   of the C-channel slice x, written to the three C-channel slices behind each other at out (out_pitch >= 3 C), one
 *   launch.  x and out may be slices of one [B, H, W, 4 C] buffer.  A NaN reaches every window that holds it.
 * bevops_upsample_nearest2x_nhwc: out [B, 2H, 2W, C] = x [B, H, W, C] at (Y / 2, X / 2). */
int bevops_focus_nhwc(const void *image, void *out, int out_pitch, int B, int H, int W, void *stream);
int bevops_spp_maxpool_nhwc(const void *x, int x_pitch, void *out, int out_pitch, int B, int H, int W, int C, int k0,
                            int k1, int k2, void *stream);
int bevops_upsample_nearest2x_nhwc(const void *x, int x_pitch, void *out, int out_pitch, int B, int H, int W, int C,
                                   void *stream);
/* bevops_conv_slice_f16's INT8 sibling (csrc/conv_slice_s8.hip; the convolutions of the INT8 build of YOLOX) on channel
 * slices of channels-last INT8 tensors, sums exact in int32 on the int8 matrix cores:
 *   sum = sum_{ky,kx,ci} x_q[b, s yo + ky - k/2, s xo + kx - k/2, ci] w_q[co, ky, kx, ci]          (int32, exact)
 * and then, every step ONE fp32 operation in exactly this order (s_aw = scale_a * scale_w and inv = 1.f / scale_out
 * are computed once on the host in fp32):
 *   sc = s_aw * w_scales[co]                (sc = s_aw when w_scales is NULL)
 *   v  = fma((float)sum, sc, bias[co])      ((float): round to nearest even, exact for |sum| <= 2^24; bias 0 when NULL)
 *   v  = act(v)                             act: 0 none, 1 ReLU max(v, 0), 2 SiLU v * rcp(1 + exp(-v)) as
 *                                           bevops_conv_slice_f16 computes it
 *   v  = fma((float)res_q, scale_res, v)    with residual_q only: the identity BEHIND the activation
 *   out_dtype BEVOPS_I8:  q = min(max(rne(v * inv), -127), 127)      BEVOPS_F16: one rounding of v to binary16
 * A NaN v leaves as -127, +inf as 127, -inf as -127 (int8); as fp16 they go through as they are.
 * x_q, residual_q and out point at the first channel of a slice (element (b, y, x, c) at base + ((b H + y) W + x)
 * pitch + c, pitches in elements); int8 slices start on 16-byte boundaries and their pitch is a multiple of 16 (an
 * fp16 out: 16-byte boundary, pitch a multiple of 8).  Every load and store lies inside its own slice: x and out may
 * be disjoint slices of one buffer, out and residual_q may be the same slice; x must not overlap out.  w_q_taps int8
 * [Cout][ksize][ksize][Cin]; w_scales fp32 [Cout], optional; bias fp32 [Cout], optional.  ksize in {1, 3}, pad ksize / 2,
 * stride in {1, 2}.  Cin % 32 == 0 (NOT 64: a thread derives the tap and channel of its own 16-byte chunk, and chunks
 * at k >= ksize^2 Cin read zero on both operands), Cout % 16 == 0 for int8 out, % 8 for fp16 out; these, ksize /
 * stride / act / out_dtype outside the lists, and B H W x_pitch or Cout ksize^2 Cin of 0xFFFFFF00 bytes or more:
 * BEVOPS_NOT_SUPPORTED.  NULL x_q / w_q_taps / out, non-positive sizes, a pitch below the channel count or no multiple
 * of 16 (8), unaligned operands, a scale in use (scale_a, scale_w; scale_res with residual_q; scale_out with int8 out)
 * that is not positive and finite: BEVOPS_BAD_PARAM.  B == 0: BEVOPS_SUCCESS without a launch.  With pitch ==
 * channels, no identity, act in {0, 1} and Cin % 64 == 0 the sums are bevops_conv_tile_int8's. */
int bevops_conv_slice_s8(const void *x_q, int x_pitch, float scale_a, const void *w_q_taps, const float *w_scales,
                         float scale_w, const float *bias, const void *residual_q, int res_pitch, float scale_res,
                         int out_dtype, void *out, int out_pitch, float scale_out, int B, int H, int W, int Cin, int Cout,
                         int ksize, int stride, int act, void *stream);
/* bevops_conv_slice_s8 with the identity IN FRONT of the activation when res_first != 0 (mmdet's BasicBlock,
 * relu(conv2(t) + identity); the INT8 build of CenterNet): the epilogue order becomes
 *   v = fma((float)sum, sc, bias[co]);  v = fma((float)res_q, scale_res, v);  v = act(v);  requantise / round
 * -- the same fp32 operations, the identity's fma moved.  res_first == 0 is bevops_conv_slice_s8 bit for bit (that
 * entry forwards here with 0).  res_first with act == 2 (SiLU) or without residual_q: BEVOPS_NOT_SUPPORTED (answered
 * after the BAD_PARAM checks and the channel-count checks of bevops_conv_slice_s8).  Everything else as there. */
int bevops_conv_slice_s8_ex(const void *x_q, int x_pitch, float scale_a, const void *w_q_taps, const float *w_scales,
                            float scale_w, const float *bias, const void *residual_q, int res_pitch, float scale_res,
                            int out_dtype, void *out, int out_pitch, float scale_out, int B, int H, int W, int Cin, int Cout,
                            int ksize, int stride, int act, int res_first, void *stream);
/* bevops_conv_slice_s8_ex with a DILATION and an optional PER-IMAGE bias (the ASPP block of the INT8 build of BEVDepth's
 * DepthNet; csrc/conv_slice_s8.hip, the same four kernels: both are block-uniform runtime values, the siblings of
 * bevops_conv_slice_f16_ex's).  bevops_conv_slice_s8_ex forwards here with (1, NULL, 0) and keeps its bits.
 *   dilation >= 1, pad = dilation * (ksize / 2): tap (ky, kx) of output pixel (y, x) reads input pixel
 *     (y + (ky - 1) dilation, x + (kx - 1) dilation), zero outside the image; stride 1 keeps the size.
 *   image_bias_f16 != NULL: fp16 [B][image_bias_pitch] in place of bias (fp16 because the few-row GEMM that makes it
 *     writes fp16, as on the fp16 path).  Output row m = pixel (b, y, x) takes the row of ITS image, b = m / (Hout Wout)
 *     -- a row tile may hold pixels of several images -- and the epilogue's first step becomes
 *       v = fma((float)sum, sc, (float)image_bias_f16[b * image_bias_pitch + co])
 *     ((float) of a binary16 value is exact); every step behind it is bevops_conv_slice_s8_ex's.
 * Statuses, in this order: everything BEVOPS_BAD_PARAM of bevops_conv_slice_s8 (NULL operands, sizes, pitches,
 * alignments, scales; out_dtype outside the list is BEVOPS_NOT_SUPPORTED in front of the pitch checks, as there);
 * dilation < 1: BEVOPS_BAD_PARAM; image_bias_f16 together with bias, image_bias_pitch < Cout, image_bias_pitch % 8 != 0 or
 * image_bias_f16 not 16-byte aligned: BEVOPS_BAD_PARAM.  Then everything BEVOPS_NOT_SUPPORTED of
 * bevops_conv_slice_s8_ex; dilation > 1 with ksize != 3 or stride != 1: BEVOPS_NOT_SUPPORTED; with dilation > 1 the
 * displacement of a tap, computed for taps outside the image too, must fit a signed 32-bit byte count:
 * dilation (W + 1) x_pitch <= 0x7FFFFFFF, else BEVOPS_NOT_SUPPORTED.  dilation == 1 is EXEMPT from this rule, so that
 * bevops_conv_slice_s8 and bevops_conv_slice_s8_ex, which forward here, keep every status they had: at dilation 1 a tap
 * inside the image lies inside the extent B H W x_pitch < 0xFFFFFF00 that is checked anyway, the kernel adds the
 * displacement to the centre pixel's offset in unsigned 32-bit arithmetic (the sum is the tap's true offset modulo
 * 2^32, whatever the displacement's size), and the value computed for a tap outside the image is never used as an
 * address.  B == 0: BEVOPS_SUCCESS without a launch. */
int bevops_conv_slice_s8_ex2(const void *x_q, int x_pitch, float scale_a, const void *w_q_taps, const float *w_scales,
                             float scale_w, const float *bias, const void *residual_q, int res_pitch, float scale_res,
                             int out_dtype, void *out, int out_pitch, float scale_out, int B, int H, int W, int Cin, int Cout,
                             int ksize, int stride, int act, int res_first, int dilation, const void *image_bias_f16,
                             int image_bias_pitch, void *stream);
/* The INT8 siblings of bevops_se_gate2_nhwc and bevops_global_avgpool_nhwc (csrc/lss_depthnet_s8.hip; the INT8 build of
 * BEVDepth's DepthNet) on int8 channel slices as in bevops_conv_slice_s8 (16-byte boundary, pitch a multiple of 16
 * elements, real = q scale).  Neither allocates, synchronises or uses atomics; n == 0: BEVOPS_SUCCESS without a launch.
 * bevops_se_gate2_nhwc_s8: x_q int8, n images of hw pixels of c channels; gates fp32 [2][n][c] as
 *   bevops_lss_camera_gate writes them.  For out_a with (gates[0], scale_a) and out_b with (gates[1], scale_b), every
 *   step ONE fp32 operation in exactly this order, none of them an addition (nothing to contract into an fma):
 *     t = (float)x_q * scale_x;   v = t * gate[i][ch];   r = v * inv_out;   q = min(max(rne(r), -127), 127)
 *   with inv_out = 1.f / scale_out computed once on the host in fp32.  A NaN r (a NaN gate) leaves as -127.  x is read
 *   once (16 bytes per thread), two 16-byte stores.  out_a / out_b must not overlap x_q or each other.
 *   Statuses, in this order: NULL operands, n < 0, hw <= 0, c <= 0; a pitch below c or no multiple of 16; x_q / gates /
 *   out_a / out_b not 16-byte aligned; a scale that is not positive and finite: BEVOPS_BAD_PARAM.  c % 16 != 0, more
 *   than 2^31 - 1 blocks of 256 vectors: BEVOPS_NOT_SUPPORTED.
 * bevops_global_avgpool_nhwc_s8: out fp16 [n][out_pitch],
 *     out[i, ch] = fp16(((float)sum * scale_x) / (float)hw),   sum = sum_p x_q[i, p, ch]   (int32, EXACT)
 *   (float)sum rounds to nearest even (exact for |sum| <= 2^24), one fp32 product, one IEEE division, one rounding to
 *   binary16.  hw <= 2^24, so |sum| <= 127 * 2^24 < 2^31.  Integer sums: the result depends on neither the order nor the
 *   grid.
 *   Statuses, in this order: NULL operands, n < 0, hw <= 0, c <= 0; x_pitch below c or no multiple of 16, out_pitch < c;
 *   x_q not 16-byte aligned, out not 2-byte aligned; scale_x not positive and finite: BEVOPS_BAD_PARAM.  c % 16 != 0,
 *   hw > 2^24, n ceil(c / 64) > 2^31 - 1: BEVOPS_NOT_SUPPORTED. */
int bevops_se_gate2_nhwc_s8(const void *x_q, int x_pitch, float scale_x, const float *gates, void *out_a, int a_pitch,
                            float scale_a, void *out_b, int b_pitch, float scale_b, int n, int hw, int c, void *stream);
int bevops_global_avgpool_nhwc_s8(const void *x_q, int x_pitch, float scale_x, void *out, int out_pitch, int n, int hw,
                                  int c, void *stream);
/* bevops_deconv4x4s2_f16's INT8 sibling (csrc/deconv_s8.hip; the up-sampling layers of the INT8 build of CenterNet):
 * ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1) + bias + ReLU on channels-last INT8 activations as four implicit
 * GEMMs on the int8 matrix cores, one per output parity, sums exact in int32:
 *   sum[b, 2y+py, 2x+px, co] = sum_{dy,dx in {0,1}} sum_ci x_q[b, y-1+py+dy, x-1+px+dx, ci] w_q[ci, co, 3-py-2dy, 3-px-2dx]
 * and then bevops_conv_slice_s8's epilogue without an identity, every step ONE fp32 operation in exactly this order
 * (s_aw = scale_a * scale_w and inv = 1.f / scale_out computed once on the host in fp32):
 *   sc = s_aw * w_scales[co]                (sc = s_aw when w_scales is NULL)
 *   v  = fma((float)sum, sc, bias[co])      ((float) exact for |sum| <= 2^24; bias 0 when NULL)
 *   v  = max(v, 0)                          with relu
 *   out_dtype BEVOPS_I8:  q = min(max(rne(v * inv), -127), 127)      BEVOPS_F16: one rounding of v to binary16
 * A NaN v leaves as -127, +inf as 127, -inf as -127 (int8); as fp16 they go through as they are.
 * x_q int8 [B, H, W, Cin]; out [B, 2H, 2W, Cout] int8 or fp16; packed_w_q the int8 weight [Cin, Cout, 4, 4] in the
 * parity-major order of bevops_deconv4x4s2_f16, [parity 2 py + px][Cout][dy][dx][Cin]; w_scales fp32 [Cout] (the
 * per-channel axis of a transposed convolution's weight is dimension 1), optional; bias fp32 [Cout], optional.
 * Cin % 64 == 0 (a 64-byte k-step never straddles two taps), Cout % 16 == 0 for int8 out, % 8 for fp16 out, out_dtype
 * outside {BEVOPS_I8, BEVOPS_F16}, B H W Cin or the packed weight (16 Cin Cout) of 0xFFFFFF00 bytes or more:
 * BEVOPS_NOT_SUPPORTED.  NULL or not 16-byte aligned x_q / packed_w_q / out, bias / w_scales not 4-byte aligned,
 * non-positive sizes, a scale in use (scale_a, scale_w; scale_out with int8 out) that is not positive and finite:
 * BEVOPS_BAD_PARAM.  B == 0: BEVOPS_SUCCESS without a launch.  (bevops_deconv4x4s2_f16 keeps refusing BEVOPS_I8.) */
int bevops_deconv4x4s2_s8(const void *x_q, float scale_a, const void *packed_w_q, const float *w_scales, float scale_w,
                          const float *bias, int out_dtype, void *out, float scale_out, int B, int H, int W, int Cin,
                          int Cout, int relu, void *stream);
/* The data-movement layers of YOLOX on INT8 slices (csrc/yolox.hip): 16-byte vectors of 16 channels, pitches multiples
 * of 16, C % 16 == 0; statuses as the fp16 entries above (a scale that is not positive and finite: BEVOPS_BAD_PARAM).
 * bevops_focus_nhwc_q: bevops_focus_nhwc from the planar fp16 image to an int8 slice of 32 channels,
 *   q = min(max(rne(x * (1.f / scale)), -127), 127), the product in fp32; channels 12 .. 31 = 0.
 * bevops_spp_maxpool_nhwc_s8: the three pools on signed bytes; padding -128 (a window always holds its centre).
 * bevops_upsample_nearest2x_nhwc_s8: a byte copy.  The pools and the copy are exact and keep their input's scale. */
int bevops_focus_nhwc_q(const void *image, float scale, void *out, int out_pitch, int B, int H, int W, void *stream);
int bevops_spp_maxpool_nhwc_s8(const void *x, int x_pitch, void *out, int out_pitch, int B, int H, int W, int C, int k0,
                               int k1, int k2, void *stream);
int bevops_upsample_nearest2x_nhwc_s8(const void *x, int x_pitch, void *out, int out_pitch, int B, int H, int W, int C,
                                      void *stream);
/* Decoder reference-point refinement (det2trt/models/modules/decoder.py:24-40, 93-103) as one launch:
 *   new_reference_points[q] = sigmoid((tmp[q][0], tmp[q][1], tmp[q][4]) + inverse_sigmoid(reference_points[q]))
 * on fp16 tensors, every step rounded to binary16 as the framework's op sequence rounds it (the refined points are the
 * next layer's sampling locations: bit-exact, tests/test_refine_gpu.py).  log and sigmoid are binary16 -> binary16
 * functions of one argument: the caller hands them in as tables of 65 536 fp16 entries (entry i = f(value with bit
 * pattern i)), filled by whatever defines its reference -- the host layer fills them with the framework's own ops.
 * reference_xy [n, 2] (optional) receives the (x, y) columns contiguously.  tmp [n, tmp_stride], tmp_stride >= 5. */
int bevops_refine_reference_points(int dtype, const void *tmp, const void *reference_points, void *new_reference_points,
                                   void *reference_xy, int num_query, int tmp_stride, const void *log_table,
                                   const void *sigmoid_table, void *stream);
/* The head's box decoding on the stacked decoder levels (det2trt/models/dense_heads/bevformer_head.py:247-282 with
 * mmdet's inverse_sigmoid): x / y / z columns (0, 1, 4) = sigmoid(reg + inverse_sigmoid(ref)) * scale + offset, the
 * other seven columns copied; every step rounded to binary16 as the framework's op sequence rounds it, log / sigmoid
 * from the caller's tables (see bevops_refine_reference_points).  regs, out [count, 10]; refs [count, 3]. */
int bevops_decode_boxes(int dtype, const void *regs, const void *refs, void *out, int count, float scale_x, float offset_x,
                        float scale_y, float offset_y, float scale_z, float offset_z, const void *log_table,
                        const void *sigmoid_table, void *stream);
/* The same convolution as an INT8 layer (`Conv2dQ`, det2trt/models/utils/register.py:79): fp16 activation
 * quantised with scale_a inside the operand load (as bevops_linear_int8_fused), int8 weights in the taps-major
 * layout, int32 sums, de-quantising epilogue with fp32 bias / fp16 identity / ReLU, fp16 out.  Cin % 64 == 0. */
int bevops_conv_tile_int8_fused(const void *x_f16, float scale_a, const void *w_q_taps, const float *w_scales,
                                float scale_w, const float *bias, const void *residual, void *out, int B, int H,
                                int W, int Cin, int Cout, int ksize, int stride, int relu, void *stream);
/* The INT8 engine's int8 ACTIVATION CHAIN (not plugins -- what TensorRT builds from the
 * reference's `Conv2dQ` / `LinearQ` layers, det2trt/models/utils/register.py:78-84, selected by
 * configs/bevformer/plugin/bevformer_base_trt_p2_q.py, when it keeps the tensors BETWEEN the layers of a ResNet
 * bottleneck in int8): every producer requantises with its consumer's calibrated input scale, so a layer moves one
 * byte per element in and one out.
 *   bevops_linear_int8_chain: bevops_linear_int8 / _fused behind one entry, plus int8 identity rows:
 *                         a [M, K] BEVOPS_I8 (quantised with scale_a) or BEVOPS_F16 (quantised in the operand load);
 *                         residual [M, N] BEVOPS_F16, or BEVOPS_I8 with scale_res (int8 `a` only); out fp16, or int8
 *                         requantised with scale_out: q = clamp(rne(v * (1 / scale_out)), -127, 127).
 *   bevops_conv_tile_int8:   bevops_conv_tile_int8_fused on an activation that already IS int8 [B, H, W, Cin]
 *                         (ksize in {1, 3}, pad ksize / 2, any stride, Cin % 64 == 0), fp16 or int8 out [B, Ho, Wo,
 *                         Cout]; `residual` must be NULL.
 *   bevops_bias_relu_maxpool_nhwc_int8: bevops_bias_relu_maxpool_nhwc leaving as int8 with scale_out (the stem
 *                         epilogue: first tensor of the chain).
 *   bevops_mdconv_forward_int8_nhwc: the DCNv2 block of the chain.  Its arithmetic is the INT8 plugin's
 *                         (modulatedDeformableConv2dKernel.cu:463-607,897-978: u8 x255 area weights, dot4 blend,
 *                         T2int8(t / 255), T2int8(val * mask), s8 x s8 -> i32 GEMM, one requantisation) on
 *                         input int8 [B, H, W, Cin] and on the offsets / sigmoid(mask logits) of the raw fp16
 *                         [B, Ho, Wo, offset_mask_channels] output of the pack's offset convolution (cnn/dcn.py:
 *                         70-86), quantised with scale_offset / scale_mask while they are staged (the Q node
 *                         TensorRT places in front of the plugin); weights packed by bevops_mdconv_pack_weight(
 *                         BEVOPS_I8); output int8 [B, Ho, Wo, Cout] with the ReLU folded into the requantisation.
 *                         exact != 0: exactly that arithmetic (bit-identical to the plugin on those operands);
 *                         exact == 0 (the engine's default): the mask is folded into the four area weights before
 *                         they are quantised, a_q = u8(area_q mask 255), so a column element is requantised ONCE,
 *                         T2int8(sum a_q v_q / 255) -- the plugin's float mask multiply + second rounding, which
 *                         makes its kernel VALU-bound, disappears; within a step of the exact flavour.
 *                         `workspace` (optional, bevops_mdconv_int8_nhwc_workspace_size() bytes) holds the int32
 *                         partial sums of the split-K tail.  NOT_SUPPORTED outside (Cin / groups) % 128 == 0, one
 *                         deform group per conv group, 3 Kh Kw <= 32. */
int bevops_linear_int8_chain(const void *a, int a_dtype, float scale_a, const void *w_q, const float *w_scales,
                             float scale_w, const float *bias, const void *residual, int res_dtype, float scale_res,
                             int out_dtype, void *out, float scale_out, long long M, int N, int K, int relu,
                             void *stream);
int bevops_conv_tile_int8(const void *x_q, float scale_a, const void *w_q_taps, const float *w_scales, float scale_w,
                          const float *bias, const void *residual, int out_dtype, void *out, float scale_out, int B,
                          int H, int W, int Cin, int Cout, int ksize, int stride, int relu, void *stream);
int bevops_bias_relu_maxpool_nhwc_int8(int dtype, const void *x, const void *bias, void *out_q, float scale_out,
                                       int n, int h, int w, int channels, void *stream);
size_t bevops_mdconv_int8_nhwc_workspace_size(void);
int bevops_mdconv_forward_int8_nhwc(const void *input_nhwc, float scale_in, const void *offset_mask_nhwc,
                                    int offset_mask_channels, float scale_offset, float scale_mask,
                                    const void *packed_weight, float scale_weight, const float *bias,
                                    void *output_nhwc, float scale_out, int relu, int exact, void *workspace,
                                    size_t workspace_bytes, int B, int Cin, int H, int W, int Cout, int Kh, int Kw,
                                    int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                                    int groups, int deform_groups, void *stream);
/* Camera-image front end of the frame loop (not a plugin): the reference's test
 * pipeline NormalizeMultiviewImage + PadMultiViewImage(size_divisor=32) + DefaultFormatBundle3D
 * (configs/bevformer/bevformer_base.py:11,228-231; third_party/bev_mmdet3d/datasets/pipelines/
 * transform_3d.py:99-150; mmcv.imnormalize) in one pass.  `images` [N, H0, W0, 3] BEVOPS_U8 or
 * BEVOPS_F32 (BGR as loaded) -> `output` [N, 3, Hp, Wp] (channels_last: [N, Hp, Wp, 3]) BEVOPS_F16
 * or BEVOPS_F32 = ((x [swapped to RGB if to_rgb] - mean[c]) * (1 / std[c])), zeros in the padding
 * rows / columns (Hp >= H0, Wp >= W0).  mean_host / std_host: 3 doubles on the HOST (mmcv keeps them
 * as float64: x - float32(mean), times float32(1 / float64(std))). */
int bevops_image_normalize_pad(int in_dtype, const void *images, int out_dtype, void *output, int N,
                               int H0, int W0, int Hp, int Wp, const double *mean_host,
                               const double *std_host, int to_rgb, int channels_last, void *stream);
/* BEVDet's camera front end (design/image_prepare.md; not a plugin): the test branch of PrepareImageInputs
 * (third_party/bev_mmdet3d/datasets/pipelines/loading.py:747-754, :691-699) in ONE launch, BIT-EXACT to PIL:
 * `images` [N, H0, W0, 3] BEVOPS_U8 (RGB, as np.array(Image.open(f)) gives them) -> Image.resize((resize_w, resize_h))
 * (Pillow's default antialiased bicubic, 8 bits per channel: 22-bit fixed-point coefficients, int32 sums, the
 * horizontal pass first, clip to uint8 after each pass) -> crop (x0, y0, x1, y1) of the resized image -> left-right
 * flip of the cropped columns if `flip` -> `canvas_or_null` [N, fH, fW, 3] uint8 (fH = y1 - y0, fW = x1 - x0) and
 * `output` [N, 3, fH, fW] (channels_last: [N, fH, fW, 3]) BEVOPS_F16 / BEVOPS_F32 = mmcv.imnormalize of the canvas,
 * as bevops_image_normalize_pad computes it (to_rgb swaps R and B: mmlabNormalize's order).
 * The PLAN holds Pillow's precompute_coeffs for both axes, restricted to the cropped columns / rows, as int32 words:
 *   [16 header: magic, H0, W0, resize_w, resize_h, x0, y0, x1, y1, ksize_x, ksize_y, window_w, window_h, 32, 16, 0]
 *   [fW][2] (first source column, taps)  [fW][ksize_x] coefficients  [fH][2] (first source row, taps)  [fH][ksize_y]
 * bevops_image_resize_plan_build is a PURE HOST function (doubles, no fused multiply-add, Pillow's operation order)
 * that fills caller-owned host memory of bevops_image_resize_plan_size bytes; the caller uploads it once per
 * geometry (4-byte aligned) and the per-frame call only launches: no allocation, no synchronisation, capturable.
 * DOMAIN: N in 1 .. 65535; all sizes in 1 .. 2^20; the crop non-empty and inside the resized image (PIL would
 * zero-fill outside: NOT_SUPPORTED); rotate == 0; and the LDS footprint of one 32 x 16 output tile -- its source
 * window (+ 3 bytes a row), the uint8 intermediate of that window's rows and the tile's coefficients -- at most
 * 64 KiB.  Every per-axis in / out ratio from 1/4 to 4 is inside (at 4: 80 window rows of 436 + 96 bytes and 3.3 KB
 * of coefficients, 45 KB); larger ratios are inside when the images are small.  Every coefficient must also fit the
 * kernel's 24-bit multiplier (|k| < 2^23, a normalised weight below 2: no bicubic geometry is known to miss it);
 * plan_size and plan_build evaluate that same check BEFORE anything is written, so they agree.  plan_size returns 0
 * outside the domain; the calls return NOT_SUPPORTED / BAD_PARAM before any device call, and BAD_PARAM unless
 * plan_bytes == bevops_image_resize_plan_size(same geometry).  The 16 header words are INFORMATIONAL: they let a
 * host program tell what a stored plan was built for; the device reads the tables only and checks neither the magic
 * nor the geometry words, so the call trusts that plan_dev is the upload of a plan that plan_build returned
 * BEVOPS_SUCCESS for with the SAME geometry arguments. */
size_t bevops_image_resize_plan_size(int H0, int W0, int resize_w, int resize_h, int crop_x0, int crop_y0,
                                     int crop_x1, int crop_y1);
int bevops_image_resize_plan_build(int H0, int W0, int resize_w, int resize_h, int crop_x0, int crop_y0, int crop_x1,
                                   int crop_y1, void *plan_host, size_t plan_bytes);
int bevops_image_resize_crop_normalize(const void *images, const void *plan_dev, size_t plan_bytes, int out_dtype,
                                       void *output, void *canvas_or_null, int N, int H0, int W0, int resize_w,
                                       int resize_h, int crop_x0, int crop_y0, int crop_x1, int crop_y1, int rotate,
                                       const double *mean_host, const double *std_host, int to_rgb, int flip,
                                       int channels_last, void *stream);
/* BEVFormer tiny / small camera front end (design/image_scale.md; not a plugin): NormalizeMultiviewImage ->
 * RandomScaleImageMultiViewImage(scales=[s]) -> PadMultiViewImage (configs/bevformer/bevformer_tiny.py:19-20,229-231,
 * bevformer_small.py:19,231-233; third_party/bev_mmdet3d/datasets/pipelines/transform_3d.py:404-438) in ONE launch.
 * `images` [N, H0, W0, 3] BEVOPS_U8 or BEVOPS_F32 (BGR as loaded) -> every tap normalised as
 * bevops_image_normalize_pad computes it -> float32 bilinear resize to [Hs, Ws] in the operation order of
 * cv::resize(INTER_LINEAR): per axis scale = 1 / (double(out) / double(in)), position f = float32((d + 0.5) * scale -
 * 0.5) (double arithmetic, one rounding), tap i = floor(f), f -= i; i < 0: i = 0, f = 0; i >= in - 1: i = in - 1,
 * f = 0 (second tap clamped to in - 1); weights (1 - f, f); one pass = fl(fl(a * w0) + fl(b * w1)), never contracted;
 * the HORIZONTAL pass first, the vertical pass on its float32 result; in == 2 * out in BOTH axes takes the area form
 * fl(fl(fl(fl(a + b) + c) + d) * 0.25f) (a, b upper source row, c, d lower) -> zero padding bottom / right to
 * [Hp, Wp] -> `output` [N, 3, Hp, Wp] (channels_last: [N, Hp, Wp, 3]) BEVOPS_F16 (its own rounding of the fp32 value)
 * or BEVOPS_F32.  Parity against cv2 itself is UNPINNED; the contract is the numpy restatement of this order in
 * tests/util_image_scale.py, bit for bit.  At Hs == H0, Ws == W0 the result equals bevops_image_normalize_pad's.
 * One launch, no workspace, no allocation, no synchronisation, capturable; coefficients are evaluated on the device.
 * DOMAIN: N in 1 .. 65535; sizes in 1 .. 2^20; the LDS footprint of one 64 x 8 output tile -- its uint8 source window
 * (+ 6 bytes a row) and the float32 horizontal-pass result of that window's rows (768 bytes a row; none in the area
 * form) -- at most 64 KiB: every per-axis ratio in / out from 1/2 to 4 is inside for both input types (at 4 in both
 * axes: 34 window rows of 780 + 768 bytes = 52 KB); larger ratios are inside while the images are small.
 * BAD_PARAM: null pointers, non-positive sizes, Hp < Hs, Wp < Ws, std <= 0, misaligned output;  NOT_SUPPORTED: other
 * dtypes, geometry outside the domain; every status is returned before any device call. */
int bevops_image_normalize_resize_pad(int in_dtype, const void *images, int out_dtype, void *output, int N,
                                      int H0, int W0, int Hs, int Ws, int Hp, int Wp, const double *mean_host,
                                      const double *std_host, int to_rgb, int channels_last, void *stream);
/* Camera front end of the two 2-D detectors (design/letterbox.md; not a plugin): mmdet's test pipelines of YOLOX
 * (configs/yolox/yolox_x_8x8_300e_coco.py:75-92: Resize(keep_ratio) -> Pad(pad_to_square, 114)) and CenterNet
 * (configs/centernet/centernet_resnet18_dcnv2_140e_coco.py:69-110: Resize(keep_ratio) -> RandomCenterCropPad(test_mode,
 * logical_or 31, a CENTRED paste) -> Pad -> Normalize) in ONE launch: resize, paste at an offset into a constant canvas,
 * normalise.  `images` [N, H0, W0, 3] BEVOPS_U8 (BGR as loaded) -> bilinear resize to [Hs, Ws] -> rows oy .. oy + Hs and
 * columns ox .. ox + Ws of `output` [N, 3, Hp, Wp] (channels_last: [N, Hp, Wp, 3]) BEVOPS_F16 or BEVOPS_F32; every other
 * element is the pad value of its channel.  pad_host: 3 doubles, raw 0 .. 255 domain, in the SOURCE channel order.
 * The resized value and the pad value are normalised AFTER the resize exactly as bevops_image_normalize_pad does it:
 * optional BGR -> RGB swap, fl(x - float32(mean)), fl(. * float32(1 / float64(std))); the fp16 output is its own
 * rounding of the fp32 value.
 * Tap positions and clamps of both arithmetics are bevops_image_normalize_resize_pad's (scale = 1 / (double(out) /
 * double(in)), f = float32((d + 0.5) * scale - 0.5) in double with one rounding, i = floor(f), f -= i, both clamps, the
 * HORIZONTAL pass first).
 * arith 0 -- cv::resize's 8-bit INTER_LINEAR in fixed point (YOLOX resizes uint8): per axis a0 = rint(fl(fl(1 - f) *
 *   2048)), a1 = rint(fl(f * 2048)) (float32 products, half to even); horizontal D = S[i] * a0 + S[i1] * a1 (int32);
 *   vertical R = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2, in 0 .. 255; H0 == 2 * Hs AND
 *   W0 == 2 * Ws takes the area form (a + b + c + d + 2) >> 2; R -> float32 exactly, then normalised.
 * arith 1 -- cv::resize's float32 INTER_LINEAR (CenterNet loads to_float32): source -> float32 exactly, one pass =
 *   fl(fl(a * w0) + fl(b * w1)) with w0 = fl(1 - f), w1 = f, never contracted; the 2 : 1 area form is
 *   fl(fl(fl(fl(a + b) + c) + d) * 0.25f); then normalised (bevops_image_normalize_resize_pad normalises every tap
 *   BEFORE the resize: the order is observable).
 * Parity against cv2 / mmcv / mmdet themselves is UNPINNED; the contract is the numpy restatement of this order in
 * tests/util_letterbox.py, bit for bit.  One launch, no workspace, no allocation, no synchronisation, capturable;
 * coefficients are evaluated on the device.
 * DOMAIN: N in 1 .. 65535; sizes in 1 .. 2^20; 0 <= oy, oy + Hs <= Hp, 0 <= ox, ox + Ws <= Wp; the LDS footprint of one
 * 64 x 8 tile of the padded output -- its uint8 source window (+ 6 bytes a row) and the horizontal-pass result of that
 * window's rows (arith 0: 384 bytes a row, arith 1: 768; none in the area form) -- at most 64 KiB: every per-axis ratio
 * in / out from 1/2 to 4 is inside whatever the image size; larger ratios are inside while the images are small.
 * BAD_PARAM: null pointers, non-positive sizes, a paste outside the canvas, std <= 0, misaligned output;
 * NOT_SUPPORTED: other dtypes, another arith, geometry outside the domain; every status is returned before any device
 * call. */
int bevops_image_letterbox(int arith, const void *images, int out_dtype, void *output, int N, int H0, int W0, int Hs,
                           int Ws, int Hp, int Wp, int oy, int ox, const double *pad_host, const double *mean_host,
                           const double *std_host, int to_rgb, int channels_last, void *stream);
/* The MSDA call in two halves, for callers that sample ONE value tensor several times or want the
 * re-layout off their critical path (not a reference plugin: the plugin's enqueue is
 * bevops_msda_forward[_ws], which does both).  `packed` = the padded head-major form of `value`
 * (csrc/msda_pad.h, msda_hm4.hip), bevops_msda_packed_size() bytes, 128-byte aligned, caller-owned;
 * it depends on (dtype, shapes, bs, heads, num_query, num_point) and, for int8, on the flavour
 * (ref_dtype).  packed_size == 0 / NOT_SUPPORTED: shape outside the head-major domain (32 channels
 * per head, the instantiated (levels x points, staged levels) combinations) -- use bevops_msda_forward.
 * bevops_msda_packed_size returns 0 exactly where bevops_msda_pack_value and
 * bevops_msda_forward_prepacked return BEVOPS_NOT_SUPPORTED for the same arguments. */
size_t bevops_msda_packed_size(int dtype, const int32_t *spatial_shapes_host, int bs, int nk, int heads,
                               int channels, int num_levels, int num_query, int num_point);
int bevops_msda_pack_value(int dtype, int ref_dtype, const void *value, const int32_t *spatial_shapes_host,
                           void *packed, size_t packed_bytes, int bs, int nk, int heads, int channels,
                           int num_levels, int num_query, int num_point, void *stream);
int bevops_msda_forward_prepacked(int dtype, const void *packed, size_t packed_bytes,
                                  const int32_t *spatial_shapes_host, const void *reference_points,
                                  int ref_dtype, const void *sampling_offsets, const void *attention_weights,
                                  void *output, int bs, int nk, int heads, int channels, int num_levels,
                                  int num_query, int num_point, int points_per_group, float scale_value,
                                  float scale_offset, float scale_weight, float scale_out, int shared_offsets,
                                  void *stream);
/* out[M, N] = act(a[M, K] . weight[N, K]^T + bias[N] + residual[M, N]) -- the dense layers around the
 * sampler (value_proj / output_proj / FFN) and the 1x1 convolutions of the
 * channels-last backbone as ONE hipBLASLt GEMM whose epilogue carries shift + identity + ReLU
 * (D = relu(A B + C + bias)).  fp16 tensors, fp32 accumulate; `bias`, `residual` optional;
 * `out` may alias `residual`.  `workspace`: caller-lent, bevops_linear_workspace_size() bytes (may be
 * NULL/0: only workspace-free algorithms are then considered).  NOT_SUPPORTED if the library has
 * no algorithm for the shape -- the caller then runs its own GEMM + bevops_bias_act_nhwc. */
size_t bevops_linear_workspace_size(void);
int bevops_linear_bias_act(int dtype, const void *a, const void *weight, const void *bias,
                           const void *residual, void *out, long long M, int N, int K, int relu,
                           void *workspace, size_t workspace_bytes, void *stream);
/* The encoder's value projection written straight into the sampler's planes, and the fused SCA sampling on
 * them (round 3; not reference plugins).  bevops_value_proj_packed: value = x @ weight.T + bias
 * (spatial_cross_attention.py:754, x [num_cams * nk, embed], weight [embed, embed]) computed by the tall-skinny
 * MFMA GEMM whose epilogue stores every output row into the padded head-major planes (csrc/msda_pad.h) instead
 * of a [cams, nk, heads, 32] tensor -- the separate re-layout pass of the sampler disappears.  `packed` (>=
 * bevops_value_proj_packed_size bytes, 128-byte aligned) then feeds bevops_sca_forward_prepacked: the fused
 * SCA sampling of bevops_sca_forward (camera-shared offsets / logits, pairs with bev_mask == 0 skipped, masked
 * camera sum) on those planes; workspace >= bevops_sca_prepacked_workspace_size bytes.  Domain: 4 levels x 8
 * points, 32 channels per head, embed % 256 == 0; BEVOPS_NOT_SUPPORTED otherwise. */
size_t bevops_value_proj_packed_size(const int32_t *spatial_shapes_host, int num_cams, int nk, int heads, int channels,
                                     int num_levels, int num_query, int num_point);
int bevops_value_proj_packed(const void *x, const void *weight, const void *bias, const int32_t *spatial_shapes_host,
                             void *packed, size_t packed_bytes, int num_cams, int nk, int heads, int channels,
                             int num_levels, int num_query, int num_point, void *stream);
int bevops_value_pack_planes(const void *value, const int32_t *spatial_shapes_host, void *packed, size_t packed_bytes,
                             int num_cams, int nk, int heads, int channels, int num_levels, int num_query,
                             int num_point, void *stream);   /* the re-layout alone, from a projected value tensor */
size_t bevops_sca_prepacked_workspace_size(int num_cams, int heads, int channels, int num_query);
int bevops_sca_forward_prepacked(int dtype, const void *packed, size_t packed_bytes, const int32_t *spatial_shapes_host,
                                 const void *reference_points_cam, const void *sampling_offsets,
                                 const void *attention_weights, const void *bev_mask, void *output, int num_cams,
                                 int nk, int heads, int channels, int num_levels, int num_query, int num_point,
                                 int points_per_group, void *workspace, size_t workspace_bytes, void *stream);
/* The same sampling on a VISIBILITY PLAN (round 5).  bev_mask depends on the calibration matrices only
 * (modules/encoder.py:255-258), so which (camera, query) pairs are sampled is known per rig, not per call:
 * bevops_sca_plan_build turns the fp16 bev_mask [num_cams, num_query] into per-camera ascending lists of the visible
 * queries (`plan`: bevops_sca_plan_size bytes -- 64 of counts, the lists, 1 KB of builder scratch per camera --
 * 16-byte aligned, device memory the caller keeps for as long as the mask is valid; num_cams <= 16, num_query <= 65 535;
 * two launches, no host synchronisation: a frame loop whose calibration changes per frame captures it in the frame's
 * graph behind bevops_point_sampling), and bevops_sca_forward_planned gives every block of the sampling
 * kernel an EQUAL slice of the global (camera, query) sequence -- no empty blocks, no per-block compaction, the same
 * number of rounds on every CU -- with the results of bevops_sca_forward_prepacked (bit-identical: same arithmetic
 * per pair, same reduction).  The plan also marks the pairs whose query no other camera sees and whose weight is
 * exactly 1 (89 % of the visible pairs of the 6-camera rig): the sampler stores those rows straight into `output`
 * (1 * v + 0 = v) and the camera reduce touches only the others.  `plan` must have been built from the VALUES of the
 * `bev_mask` passed here (not only from its zero pattern); bevops_sca_forward_planned returns BEVOPS_BAD_PARAM unless
 * plan_bytes == bevops_sca_plan_size(num_cams, num_query) -- a plan built for another camera set or query count is
 * rejected (what the plan's CONTENT was built from cannot be checked without a host synchronisation and is not). */
size_t bevops_sca_plan_size(int num_cams, int num_query);
int bevops_sca_plan_build(int dtype, const void *bev_mask, int num_cams, int num_query, void *plan, size_t plan_bytes,
                          void *stream);
int bevops_sca_forward_planned(int dtype, const void *packed, size_t packed_bytes, const int32_t *spatial_shapes_host,
                               const void *reference_points_cam, const void *sampling_offsets,
                               const void *attention_weights, const void *bev_mask, const void *plan, size_t plan_bytes,
                               void *output, int num_cams, int nk, int heads, int channels, int num_levels,
                               int num_query, int num_point, int points_per_group, void *workspace,
                               size_t workspace_bytes, void *stream);

/* point_sampling_trt (det2trt/models/modules/encoder.py:197-259) as one launch (csrc/point_sampling.hip): the BEV
 * pillar anchors `pillars` [num_points_in_pillar, num_query, 4] (fp32 metric homogeneous points: the frame-independent
 * first half, encoder.py:199-219) projected with `lidar2img` [num_cams, 4, 4] (fp32, row-major, DEVICE memory: the
 * reference feeds it as an engine input on every frame, tools/bevformer/evaluate_trt.py:131-132), divided by the depth
 * and the image size -> reference_points_cam [num_cams, num_query, num_points_in_pillar, 2] and the visibility weights
 * bev_mask [num_cams, num_query] = (any anchor inside the image and in front of the camera) / max(number of cameras that
 * see the pillar, 1e-4), both in `out_dtype` (BEVOPS_F16 | BEVOPS_F32).  Index generation is bit-exact (SURVEY 8a row
 * a6): fp32 arithmetic in the reference's op order -- separately rounded products and sums in ascending k, IEEE
 * divisions -- rounded once to the output type.  BEVOPS_NOT_SUPPORTED unless num_points_in_pillar == 4. */
int bevops_point_sampling(int out_dtype, const float *pillars, const float *lidar2img, void *reference_points_cam,
                          void *bev_mask, int num_cams, int num_query, int num_points_in_pillar, float image_h,
                          float image_w, void *stream);

/* Hand-written tall-skinny fp16 GEMM on the matrix cores (csrc/tsgemm.hip) for the dense layers that wrap the
 * samplers (the reference runs them as cuBLAS / TensorRT layers: spatial_cross_attention.py:694-768,
 * backbones/resnet.py:326-686): out[m, n] = act(sum_k x[m, k] w[n, k] + bias[n] (+ residual[m, n])), x [M, K],
 * w [N, K], residual / out [M, N] row-major fp16, fp32 accumulation, one rounding.  Persistent blocks stream
 * their rows once; both operands reach LDS by DMA.  BEVOPS_NOT_SUPPORTED outside K % 64 == 0, N % 256 == 0
 * (the caller keeps its library GEMM). */
int bevops_tsgemm_f16(const void *x, const void *weight, const void *bias, const void *residual, void *out,
                      long long m, int n, int k, int relu, void *stream);
/* K <= 256 runs on the weight-stationary flavour of that kernel (weights in registers for the whole launch, activation
 * rows prefetched two tiles ahead; k ascending in every block, so an output row depends on its own operands only).
 * bevops_tsgemm_set_variant (thread-local A/B switch, like bevops_stem_set_variant): 0 = default, 1 = the original kernel
 * for every K; applies to bevops_tsgemm_f16, bevops_tsgemm_f16_ln and bevops_value_proj_packed together.  Returns the
 * previous value.  BEVOPS_TSGEMM_WS=0 in the environment when the library loads is variant 1 for every thread.
 * bevops_tsgemm_tile_rows: rows per tile of the kernel that runs for this k under the current variant (0: k outside the
 * domain). */
int bevops_tsgemm_set_variant(int variant);
int bevops_tsgemm_tile_rows(int k);
/* `groups` dense layers of 256 columns over the SAME rows as ONE launch of the weight-stationary kernel (the six
 * decoder layers' value_proj of bev_embed): weight
 * [groups * 256, K], bias [groups * 256] or NULL; layer g's result is the dense [M, 256] matrix at
 * out + g * group_stride (fp16 elements; >= m * 256, a multiple of 8).  Exactly the bytes of `groups` calls of
 * bevops_tsgemm_f16 with n = 256 -- the rows are read from HBM once instead of `groups` times.  No residual, no
 * activation.  BEVOPS_NOT_SUPPORTED unless K % 64 == 0 and K <= 256. */
int bevops_tsgemm_f16_grouped(const void *x, const void *weight, const void *bias, void *out, long long group_stride,
                              long long m, int groups, int k, void *stream);
/* The same GEMM with the LayerNorm that follows it in every encoder / decoder block (modules/encoder.py:586-636,
 * modules/decoder.py:52-112: attention or FFN with its identity, then `norm`) evaluated in the epilogue:
 *     out = LayerNorm_N(fp16(x w^T + bias (+ residual))) * ln_weight + ln_bias,     N == 256, K % 64 == 0.
 * The row is normalised from exactly the binary16 sums the unfused pair (this GEMM, then bevops_layer_norm) would have
 * read back -- fp32 mean, centred squares, one rounding -- without the second launch and the [M, 256] round trip.
 * ln_weight / ln_bias fp16 [256], 16-byte aligned.  BEVOPS_NOT_SUPPORTED when n != 256 or k % 64 != 0. */
int bevops_tsgemm_f16_ln(const void *x, const void *weight, const void *bias, const void *residual, const void *ln_weight,
                         const void *ln_bias, float eps, void *out, long long m, int n, int k, void *stream);
/* Self-attention of a few hundred queries on the matrix cores (csrc/attention.hip; the decoder's object queries:
 * mmcv MultiheadAttention in det2trt/models/modules/decoder.py:52-112 -- 900 queries, 8 heads x 32): qkv
 * [num_query, 3, heads, 32] fp16 (the in-projection's output: q, k, v of every head side by side, 16-byte aligned) ->
 * out [num_query, heads, 32] fp16 = softmax(scale q k^T) v per head; fp32 scores / statistics / accumulators.
 * BEVOPS_NOT_SUPPORTED unless head_dim == 32 and num_query <= bevops_mha_selfattn_max_queries() (the head's keys and
 * values live in LDS). */
size_t bevops_mha_selfattn_max_queries(void);
int bevops_mha_selfattn_f16(const void *qkv, void *out, int num_query, int heads, int head_dim, float scale, void *stream);
/* The int8 activation chain's flavour of the same persistent kernel (the int8 1x1 convolutions of ResNet stages
 * 3 / 4; arguments as bevops_linear_int8_chain with an int8 activation): a_q [M, K] / w_q [N, K] int8, int32 sums,
 * fp32 bias, identity rows int8 (res_dtype BEVOPS_I8, real = q * scale_res) or fp16, output int8 (requantised with
 * scale_out) or fp16.  128 k-values per step.  BEVOPS_NOT_SUPPORTED outside K % 128 == 0, N % 256 == 0.
 * The host layer uses it for the 256-column layers with K = 1 024 (ResNet stage-3 conv1), where it measured faster
 * than the tiled int8 GEMM (profiles/r04/tsgemm_s8_ab.jsonl). */
int bevops_tsgemm_s8(const void *a_q, float scale_a, const void *w_q, const float *w_scales, float scale_w,
                     const float *bias, const void *residual, int res_dtype, float scale_res, int out_dtype,
                     void *out, float scale_out, long long m, int n, int k, int relu, void *stream);
/* That kernel with the LayerNorm that ends every encoder block in its epilogue (the int8 counterpart of
 * bevops_tsgemm_f16_ln):
 *     out = LayerNorm_256(fp16(acc * scale_a * scale_w[n] + bias[n] (+ identity[m, n]))) * ln_weight + ln_bias.
 * The pre-norm value is rounded to binary16 once, exactly as bevops_tsgemm_s8 rounds its fp16 output; the row is then
 * normalised from those values with fp32 statistics (mean, centred squares, one rounding): the result is what the pair
 * bevops_tsgemm_s8 (fp16 out) -> bevops_layer_norm gives, up to the last bit of the normalisation, without the second
 * launch and the [M, 256] round trip.  No ReLU; identity int8 (with scale_res) or fp16 or NULL; w_scales fp32 [256] or
 * NULL (then scale_w); ln_weight / ln_bias fp16 [256]; out fp16 [M, 256]; a_q, w_q, ln_weight, ln_bias, out 16-byte
 * aligned.  No workspace.  BEVOPS_NOT_SUPPORTED when n != 256 or k % 128 != 0; BEVOPS_BAD_PARAM for a missing
 * ln_weight / ln_bias, !(eps >= 0) or a misaligned operand. */
int bevops_tsgemm_s8_ln(const void *a_q, float scale_a, const void *w_q, const float *w_scales, float scale_w,
                        const float *bias, const void *residual, int res_dtype, float scale_res,
                        const void *ln_weight, const void *ln_bias, float eps, void *out, long long m, int n, int k,
                        void *stream);

/* The same dense layer for problems with FEW rows (the decoder's 900 object queries: decoder.py:381-471,
 * bevformer_head.py:247-282; csrc/small_gemm.hip): 32 x 64 output tiles, split-K over the four waves of a block, every
 * operand fragment requested before the first matrix instruction -- one memory round trip per launch instead of a
 * chain of dependent k-steps.  fp16 in / out, fp32 sums, bias / residual fp16, optional.  BEVOPS_NOT_SUPPORTED outside
 * K % 64 == 0, K <= 1024, M <= 65536. */
int bevops_small_gemm_f16(const void *x, const void *weight, const void *bias, const void *residual, void *out,
                          long long m, int n, int k, int relu, void *stream);

/* OPTIONAL, BLOCKING: pick the hipBLASLt algorithm for one bevops_linear_bias_act problem (same
 * arguments) by timing every supporting algorithm on `stream` with the caller's buffers, and cache
 * it for the process.  `out` is scratch and must not alias `residual`.  Synchronises the host;
 * BAD_PARAM under stream capture.  Without it the operator runs the library heuristic's choice
 * (measured 1.5-3x slower at the backbone's shapes). */
int bevops_linear_tune(int dtype, const void *a, const void *weight, const void *bias,
                       const void *residual, void *out, long long M, int N, int K, int relu,
                       void *workspace, size_t workspace_bytes, void *stream);
int bevops_mdconv_forward_packed(int dtype, const void *input, const void *offset,
                                 const void *mask, const void *packed_weight, const void *bias,
                                 void *output, void *workspace, size_t workspace_bytes, int B,
                                 int Cin, int H, int W, int Cout, int Kh, int Kw, int stride_h,
                                 int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                                 int groups, int deform_groups, void *stream);

/* ------------------------------------------------------------------------
 * Scaled dot-product attention, QKVTRT / QKVTRT2 (csrc/qkv.hip).
 * Replaces QKVPlugin::enqueue (TensorRT/plugin/multi_head_attn/multiHeadAttnPlugin.cpp:89-150)
 * and what it computes, det2trt/models/functions/multi_head_attn.py:12-16:
 *   output[b, i, :] = sum_j softmax_j(<query[b, i, :], key[b, j, :]> / sqrt(embed_dim)) value[b, j, :]
 *   query [batch, q_len, embed_dim], key / value [batch, kv_len, embed_dim], output [batch, q_len, embed_dim]
 * F32 (f32 operands throughout) and F16 (fp32 scores, statistics and sums; probabilities rounded to binary16 for
 * the second product); any lengths >= 1; embed_dim % 16 == 0 and 16 <= embed_dim <= 128, else
 * BEVOPS_NOT_SUPPORTED.  scale_*: the INT8 per-tensor scales the plugin reads (multiHeadAttnPlugin.cpp:97-100),
 * ignored for F32 / F16; I8 is BEVOPS_NOT_SUPPORTED.  workspace: bevops_qkv_workspace_size bytes (0 = none
 * needed; more than 0 when few query tiles meet many keys and the keys are split across blocks), 16-byte aligned;
 * a NULL or short one is BEVOPS_BAD_PARAM.  No atomics: results are bit-reproducible.
 * ------------------------------------------------------------------------ */
size_t bevops_qkv_workspace_size(int dtype, int batch, int q_len, int kv_len, int embed_dim);
int bevops_qkv_forward(int dtype, const void *query, const void *key, const void *value, void *output, int batch,
                       int q_len, int kv_len, int embed_dim, float scale_q, float scale_k, float scale_v,
                       float scale_o, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Batched matrix inverse, InverseTRT (csrc/inverse.hip).
 * Replaces InversePlugin::enqueue (TensorRT/plugin/inverse/inversePlugin.cpp:58-75, inverseKernel.cu:9-41:
 * cublasSgetrfBatched + cublasSgetriBatched) and torch.linalg.inv (functions/inverse.py:11-13):
 *   output[b] = input[b]^-1, input / output [batch, n, n] F32, 1 <= n <= 32 (else, and for F16 / I8,
 *   BEVOPS_NOT_SUPPORTED).  Partial pivoting.  A matrix with an exactly zero pivot comes back all NaN and the
 *   status stays BEVOPS_SUCCESS (the plugin cannot report a failure per matrix either); the other matrices of the
 *   batch are unaffected.
 * ------------------------------------------------------------------------ */
int bevops_inverse_forward(int dtype, const void *input, void *output, int batch, int n, void *stream);

/* ------------------------------------------------------------------------
 * Detection decode (csrc/decode.hip): raw head outputs -> boxes, scores, labels.  Not reference plugins: the
 * reference runs these steps as ~30 framework launches with data-dependent shapes in `post_process`
 * (det2trt/models/detector/bevformer.py:46-49, bevdet.py:84-89).  Not to be confused with bevops_decode_boxes,
 * which is the head's sigmoid + de-normalisation of the regression output.
 *
 * Both entries write FIXED-CAPACITY outputs, so they need no host round trip and can be captured:
 *   boxes [batch, max_num, 9] F32, scores [batch, max_num] F32, labels [batch, max_num] int32, count [batch] int32.
 * The kept detections of item b are rows 0 .. count[b]-1, in rank order (what boolean-mask indexing of the
 * reference's descending top-k list gives); rows at and behind count[b] are zero.  Inputs are F32 or F16 (an F16
 * input means its values widened); all arithmetic and all outputs are F32; I8 is BEVOPS_NOT_SUPPORTED.  Inputs need
 * no particular alignment.  No atomic whose order can show in a result: outputs are bit-reproducible.
 * NULL pointers (where not stated optional), max_num < 1 and max_num above the number of candidates are
 * BEVOPS_BAD_PARAM, returned before any device call.  `*_host` arrays are read during the call only.
 *
 * RANKING RULE.  Selection ranks the candidates by their fp32 LOGIT, larger first (sigmoid is monotone, so this is
 * a top-k of the scores); equal logits (-0 equals +0) rank by LOWER FLAT INDEX first -- NMS-free:
 * query * num_classes + class; CenterPoint: class * H * W + row * W + col.  torch.topk leaves the order among
 * equals unspecified, so this is one valid reading of the reference, fixed so that results are reproducible.
 *
 * bevops_nms_free_decode: NMSFreeCoder.decode_single (third_party/bev_mmdet3d/core/bbox/coders/nms_free_coder.py:42-98,
 * denormalize_bbox core/bbox/util.py:26-53) per batch item, optionally with the z shift of BEVFormerHead.get_bboxes
 * (models/dense_heads/bevformer_head.py:556).
 *   cls_logits [batch, num_query, num_classes], bbox_preds [batch, num_query, 10] =
 *   (cx, cy, log w, log l, cz, log h, sin, cos, vx, vy); score = sigmoid(logit), label = flat index % num_classes,
 *   box = (cx, cy, cz, e^w, e^l, e^h, atan2(sin, cos), vx, vy).  Kept: centre inside post_center_range_host[6]
 *   (x, y, z lower bounds, then upper bounds, both inclusive) and the score test: score_threshold < 0 = none;
 *   otherwise score > threshold, and when no candidate of the item passes, the reference's relaxation
 *   (threshold *= 0.9 in double, test score >= threshold, until something passes; keep all once it falls below
 *   0.01), evaluated on the device.  NaN / infinite thresholds are BEVOPS_BAD_PARAM.  bottom_center = 1 applies
 *   z -= e^h / 2 AFTER the range test (the coder's output when 0).  num_query * num_classes <= 16 384, else
 *   BEVOPS_NOT_SUPPORTED.  One launch, one workgroup per batch item.
 *
 * bevops_centerpoint_decode: CenterHead.get_bboxes up to the NMS (models/dense_heads/centerpoint_head.py:716-746)
 * with CenterPointBBoxCoder.decode (core/bbox/coders/centerpoint_bbox_coders.py:138-230): the global top max_num of
 * the num_classes x H x W heat map (what the coder's two-stage top-k selects), gather of the heads at the winning
 * cells, x = (col + reg[0]) * out_size_factor * voxel_x + pc_x (y likewise with row, reg[1]; each step rounded to
 * F32 like the reference's tensor ops), box = (x, y, height, dim[0..2] (exp'd when norm_bbox), atan2(rot[0], rot[1]),
 * vel[0], vel[1]), label = class.  heatmap_is_score = 1: the map already holds scores (the coder's own `decode`
 * receives the sigmoid's output); they are ranked and reported as they are, no sigmoid is applied.  Kept: score > score_threshold (< 0 = none) and (x, y, height) inside
 * post_center_range_host.  Maps: reg [batch, 2, H, W], height [.,1,.,.], dim [.,3,.,.], rot [.,2,.,.],
 * vel [.,2,.,.], heatmap [., num_classes, ., .], each dense per batch item (item stride = channels * H * W) and read
 * in place through strides_host[12] = (channel stride, pixel stride) in elements for reg, height, dim, rot, vel,
 * heatmap: (H * W, 1) for contiguous NCHW, (1, channels) for channels-last.  vel may be NULL (box columns 7, 8
 * zero), reg may be NULL (+ 0.5).  max_num <= 4 096, else BEVOPS_NOT_SUPPORTED.  workspace:
 * bevops_centerpoint_decode_workspace_size bytes, 8-byte aligned (0 = none needed: the heat map fits one
 * workgroup's selection, one launch; otherwise two launches); a NULL or short one is BEVOPS_BAD_PARAM.
 *
 * bevops_centerpoint_decode_ex: the same call with strides_host[18] (int64) = (channel stride, pixel stride, ITEM
 * stride) in elements per map, so a batch of maps that are channel slices of one wider channels-last tensor
 * [batch, H, W, Ct] -- BEVDet's packed head output -- is read in place: (1, Ct, H * W * Ct).  Every stride >= 1, channel
 * and pixel strides below 2^31, else BEVOPS_BAD_PARAM.  bevops_centerpoint_decode is this entry with item stride =
 * channels * H * W; same kernels, same bits.
 * ------------------------------------------------------------------------ */
int bevops_nms_free_decode(int dtype, const void *cls_logits, const void *bbox_preds, float *boxes, float *scores,
                           int32_t *labels, int32_t *count, int batch, int num_query, int num_classes, int max_num,
                           const float *post_center_range_host, float score_threshold, int bottom_center,
                           void *stream);
size_t bevops_centerpoint_decode_workspace_size(int batch, int num_classes, int height, int width, int max_num);
int bevops_centerpoint_decode(int dtype, const void *reg, const void *height, const void *dim, const void *rot,
                              const void *vel, const void *heatmap, const int32_t *strides_host, float *boxes,
                              float *scores, int32_t *labels, int32_t *count, int batch, int num_classes, int map_h,
                              int map_w, int max_num, float out_size_factor, float voxel_x, float voxel_y, float pc_x,
                              float pc_y, const float *post_center_range_host, float score_threshold, int norm_bbox,
                              int heatmap_is_score, void *workspace, size_t workspace_bytes, void *stream);
int bevops_centerpoint_decode_ex(int dtype, const void *reg, const void *height, const void *dim, const void *rot,
                                 const void *vel, const void *heatmap, const int64_t *strides_host, float *boxes,
                                 float *scores, int32_t *labels, int32_t *count, int batch, int num_classes, int map_h,
                                 int map_w, int max_num, float out_size_factor, float voxel_x, float voxel_y,
                                 float pc_x, float pc_y, const float *post_center_range_host, float score_threshold,
                                 int norm_bbox, int heatmap_is_score, void *workspace, size_t workspace_bytes,
                                 void *stream);

/* ------------------------------------------------------------------------
 * BEV non-maximum suppression (csrc/nms.hip): what CenterHead.get_bboxes does behind the coder
 * (third_party/bev_mmdet3d/models/dense_heads/centerpoint_head.py:747-806) -- the rotated "scale-NMS" of
 * get_task_detections (:808-905) through nms_bev (core/post_processing/box3d_nms.py:227-273), or circle_nms
 * (box3d_nms.py:182-221), then the size restore (:870-876) and the z shift to the bottom centre (:793).
 *
 * bevops_bev_nms.  mode 0 = rotate (row j is suppressed by an earlier kept row i when IoU(i, j) > threshold,
 * strictly), 1 = circle (when (x_i - x_j)^2 + (y_i - y_j)^2 <= threshold).
 *   boxes_in [batch, num, 9] F32 = (x, y, z, w, l, h, yaw, vx, vy) as bevops_centerpoint_decode writes them, scores_in
 *   [batch, num] F32, labels_in [batch, num] int32, count_in [batch] int32 = valid rows per item, read ON THE DEVICE
 *   (NULL = num; above num is read as num, below 0 as 0).  Rows at and behind count_in[b] are never read as
 *   candidates, whatever they hold.
 *   Outputs, fixed capacity like the decoders': boxes [batch, post_max_size, 9], scores, labels [batch, post_max_size],
 *   count [batch], index [batch, post_max_size] int32 = the kept rows as row numbers of the input (may be NULL); kept
 *   rows first, in rank order, everything at and behind count[b] zero.  No host round trip: capturable.
 * RANK (nms_bev :249-253, circle_nms :202): the valid rows in descending score order, cut to pre_max_size (<= 0 = no
 *   cut).  Equal scores (-0 equals +0) rank by LOWER INPUT ROW first: the decoders' rule, the same 64-bit key.
 * SCALE (centerpoint_head.py:836-844): w, l, h of a row with label c are multiplied by rescale_factor_host[c] in F32
 *   (num_factors = 1: every row by rescale_factor_host[0]; 0: no scaling; labels outside [0, num_factors) are left
 *   alone).  The pair test sees (x, y, w f, l f, yaw), the `.bev` columns 0, 1, 3, 4, 6 (lidar_box3d.py:94;
 *   xyxyr2xywhr=False at centerpoint_head.py:865), w along (cos yaw, sin yaw).  At most 64 factors.
 * PAIR TEST, rotate: intersection area of the two rotated rectangles over area_i + area_j - intersection -- nms_bev's
 *   "exact overlapping area" -- evaluated in F32 in the frame of box i (rectangle j clipped against the four edges of
 *   rectangle i, coordinates relative to i's centre); a pair whose union is not positive has IoU 0; a row with a
 *   non-finite x, y, w, l or yaw suppresses nothing and is not suppressed.  bevops_bev_iou exposes this function;
 *   its distance from the F64 value is bounded by a test at 5e-4 and measured near 1e-6 (design/postprocess.md).
 * PAIR TEST, circle: the squared distance in F32, each operation rounded on its own, compared with `threshold` AS IT
 *   IS: circle_nms compares min_radius with the SQUARED distance (:216-219), so min_radius is not squared here either.
 * SCAN: in rank order, a row not yet suppressed is kept and suppresses; stops after post_max_size kept rows.
 * WRITE: columns 0-2, 6-8, score and label are copied bits.  With factors, columns 3-5 are fl(fl(d f) / f), IEEE F32
 *   division: the reference multiplies in place and divides back, which does not always return d.  bottom_center != 0:
 *   then z = fl(z - fl(h 0.5)) with that h.
 * LIMITS, checked before any device call: batch >= 1, 1 <= num <= 4 096 (above: BEVOPS_NOT_SUPPORTED, as are more
 *   than 64 factors), 1 <= post_max_size <= num; NULL pointers (index and count_in excepted), a workspace shorter than
 *   bevops_bev_nms_workspace_size(batch, num) or not 8-byte aligned, a non-finite threshold or factor, a factor <= 0:
 *   BEVOPS_BAD_PARAM.  Three launches (rank + scale; suppression matrix as 64-bit words, one wave per word; scan +
 *   gather), none sized by a device value.  Outputs are bit-reproducible.
 *
 * bevops_bev_iou: iou [num_a, num_b] F32 of boxes_a [num_a, 5] and boxes_b [num_b, 5], (x, y, w, l, yaw) each,
 * evaluated in the frame of the a-box; NaN where a box has a non-finite entry.  num_a * num_b <= 2^30.
 * ------------------------------------------------------------------------ */
size_t bevops_bev_nms_workspace_size(int batch, int num);
int bevops_bev_nms(int mode, const float *boxes_in, const float *scores_in, const int32_t *labels_in,
                   const int32_t *count_in, float *boxes, float *scores, int32_t *labels, int32_t *count,
                   int32_t *index, int batch, int num, int pre_max_size, int post_max_size, float threshold,
                   const float *rescale_factor_host, int num_factors, int bottom_center, void *workspace,
                   size_t workspace_bytes, void *stream);
int bevops_bev_iou(const float *boxes_a, int num_a, const float *boxes_b, int num_b, float *iou, void *stream);

/* ------------------------------------------------------------------------
 * 2-D detection decode (csrc/decode2d.hip; bevops_box_nms in csrc/nms.hip): the post-processing of the reference's two 2-D detectors
 * (det2trt/models/detector/centernet.py, yolox.py: post_process with rescale=True), which it runs as framework ops with
 * data-dependent shapes.  The statement below is the published algorithm of mmdet 2.x (CenterNetHead.get_bboxes /
 * decode_heatmap, YOLOXHead.get_bboxes / _bbox_decode / _bboxes_nms) and of mmcv.ops.batched_nms / nms.  Neither
 * library is part of this project's test environment, so parity with the libraries themselves is UNPINNED
 * (design/postprocess.md); what is pinned is this statement, through an independent numpy restatement.
 *
 * As the "Detection decode" entries above: FIXED-CAPACITY outputs, no host round trip, no launch sized by a device
 * value, capturable, bit-reproducible (no atomic whose order can show in a result).  Map inputs are F32 or F16 (F16
 * values widened), I8 is BEVOPS_NOT_SUPPORTED; all arithmetic and all outputs are F32 (labels, count, index int32).
 * Each map is dense per batch item and read in place through (channel stride, pixel stride) pairs in elements:
 * (H * W, 1) for contiguous NCHW, (1, channels) for channels-last.  Inputs need no particular alignment.  F32
 * arithmetic is written operation by operation, each rounded once, never contracted into an FMA; divisions are IEEE.
 * `*_host` arrays are read during the call only.  Per-image host values travel as kernel arguments: batch <= 64 for the
 * two decoders, else BEVOPS_NOT_SUPPORTED.  NULL pointers (where not stated optional) are BEVOPS_BAD_PARAM.  All checks
 * happen on the host before any device call.
 *
 * bevops_centernet_decode.  heatmap [batch, C, H, W] holds SCORES (the head applied the sigmoid; none is applied here),
 * wh [batch, 2, H, W], offset [batch, 2, H, W]; strides_host[6] = the pairs of heatmap, wh, offset.
 *   LOCAL MAXIMUM: a cell keeps its value when no cell of its kernel x kernel window, clipped to the image, is greater
 *   (max_pool2d, stride 1, -inf padding, hmax == heat); otherwise its value is +0.  A kept -0 counts as +0.  kernel is
 *   1, 3, 5 or 7; other sizes are BEVOPS_NOT_SUPPORTED (even or < 1 included; < 1 is BEVOPS_BAD_PARAM).
 *   TOP k: the thinned values of the C H W cells under the RANKING RULE above -- larger value first, equal values (the
 *   many exact zeros included) by lower flat index c H W + y W + x first.  label = index / (H W), y and x from the rest.
 *   BOX: xs = x + offset0, ys = y + offset1; tl_x = (xs - wh0 / 2) rx, br_x = (xs + wh0 / 2) rx, y likewise with wh1 and
 *   ry; rx = (float)((double)inp_w / W), ry = (float)((double)inp_h / H).  Then x -= border_host[b][0],
 *   y -= border_host[b][1] (border_host [batch, 2] = mmdet's border[2], border[0]; NULL = none); then, when
 *   scale_factor_host [batch, 4] is not NULL, the four columns are divided by it (mmdet's rescale).
 *   OUTPUT: boxes [batch, k, 4] (tl_x, tl_y, br_x, br_y), scores [batch, k], labels [batch, k], count [batch], in rank
 *   order.  score_threshold < 0 (mmdet: none): count = k.  Otherwise rows with score > score_threshold are kept,
 *   compacted to the front, zeros behind.
 *   NaN: a NaN cell is never greater and nothing is greater than it, so it is kept, suppresses nothing, and ranks by
 *   its bits (a positive NaN before +inf, a negative NaN last); its score is written as it is.  Stays inside the buffers.
 *   LIMITS: 1 <= k <= min(4 096, C H W) and C H W <= 2^24, else BEVOPS_NOT_SUPPORTED; a workspace that is NULL,
 *   shorter than bevops_centernet_decode_workspace_size or not 8-byte aligned, a NaN threshold, a non-finite or zero
 *   scale factor, a non-finite border, a stride < 1: BEVOPS_BAD_PARAM.  The size query is 0 exactly where the entry
 *   answers BEVOPS_NOT_SUPPORTED for its dimensions (or the dimensions are < 1).  Two launches.
 *
 * bevops_yolox_decode.  num_levels (1 .. 8) levels; level l: cls_host[l] -> [batch, C, H_l, W_l], bbox_host[l] ->
 * [batch, 4, H_l, W_l], obj_host[l] -> [batch, 1, H_l, W_l] device pointers, all LOGITS; level_shapes_host [L, 3] =
 * (H_l, W_l, stride_l); strides_host [L, 6] = the pairs of cls, bbox, obj.
 *   PRIORS: cell (row, col) of level l has the prior (col stride_l, row stride_l) (MlvlPointGenerator, offset 0);
 *   priors are numbered level-major, then row, then column, P in all (P <= 2^24).
 *   BOX: cx = p0 stride + prior_x, cy = p1 stride + prior_y, w = exp(p2) stride, h = exp(p3) stride, x1 = cx - w / 2,
 *   y1 = cy - h / 2, x2 = cx + w / 2, y2 = cy + h / 2; then, when scale_factor_host [batch, 4] is not NULL, divided by
 *   it (mmdet rescales BEFORE the NMS).
 *   SCORE: sigmoid(obj) * sigmoid(largest class logit); label = argmax of the F32 class LOGIT, ties to the lower class
 *   (a NaN logit of a class > 0 never wins).  DEVIATION: mmdet takes the argmax after the sigmoid, which differs only
 *   where the sigmoid saturates and ties logits that differ.
 *   OUTPUT, in prior order, no compaction, no threshold (bevops_box_nms applies it): boxes [batch, P, 4], scores
 *   [batch, P], labels [batch, P].  One launch.
 *
 * bevops_box_nms: the axis-aligned batched_nms.
 *   boxes_in [batch, num, 4] F32 (x1, y1, x2, y2), scores_in [batch, num] F32, labels_in [batch, num] int32, count_in
 *   [batch] int32 read ON THE DEVICE (NULL = num; above num is read as num, below 0 as 0).
 *   CANDIDATES: rows below count_in[b] with score >= score_threshold (mmdet's valid_mask; -inf = every row; a NaN
 *   score is no candidate).  RANK: descending score, equal scores (-0 equals +0) by LOWER INPUT ROW first.
 *   PAIR TEST, F32, in this order: area = (x2 - x1) (y2 - y1); iw = max(min(x2_i, x2_j) - max(x1_i, x1_j), 0), ih
 *   likewise; inter = iw ih; iou = inter / ((area_i + area_j) - inter).  Row j is suppressed by an earlier kept row i
 *   when iou > iou_threshold (strictly; a NaN iou suppresses nothing) and, with class_aware = 1, label_i == label_j.
 *   A row with a non-finite coordinate suppresses nothing and is not suppressed.
 *   DEVIATION: mmcv realises class-awareness by adding label (max_coordinate + 1) to the coordinates, which perturbs
 *   their low bits and lets boxes with negative coordinates leak across classes.  That is NOT restated: the label
 *   test is the definition here.
 *   OUTPUT as bevops_bev_nms: kept rows first, in rank order, at most max_out of them, into boxes [batch, max_out, 4],
 *   scores, labels [batch, max_out], count [batch], index [batch, max_out] (input row numbers; may be NULL);
 *   everything at and behind count[b] is zero.  Kept rows are copied bits.
 *   LIMITS: 1 <= num <= 16 384 (above: BEVOPS_NOT_SUPPORTED, and the size query is 0), 1 <= max_out <= num,
 *   class_aware 0 or 1; a NaN score_threshold, a non-finite iou_threshold, a workspace that is NULL, shorter than
 *   bevops_box_nms_workspace_size(batch, num) or not 8-byte aligned: BEVOPS_BAD_PARAM.  The workspace holds the
 *   suppression matrix for the worst case, num^2 / 8 bytes per item (32 MiB at 16 384 rows); only the part the
 *   candidates need is written and read.  Three launches.
 * ------------------------------------------------------------------------ */
size_t bevops_centernet_decode_workspace_size(int batch, int num_classes, int height, int width, int k);
int bevops_centernet_decode(int dtype, const void *heatmap, const void *wh, const void *offset,
                            const int32_t *strides_host, float *boxes, float *scores, int32_t *labels, int32_t *count,
                            int batch, int num_classes, int map_h, int map_w, int k, int kernel, int inp_h, int inp_w,
                            const float *border_host, const float *scale_factor_host, float score_threshold,
                            void *workspace, size_t workspace_bytes, void *stream);
int bevops_yolox_decode(int dtype, const void *const *cls_host, const void *const *bbox_host,
                        const void *const *obj_host, const int32_t *level_shapes_host, const int32_t *strides_host,
                        float *boxes, float *scores, int32_t *labels, int batch, int num_levels, int num_classes,
                        const float *scale_factor_host, void *stream);
size_t bevops_box_nms_workspace_size(int batch, int num);
int bevops_box_nms(const float *boxes_in, const float *scores_in, const int32_t *labels_in, const int32_t *count_in,
                   float *boxes, float *scores, int32_t *labels, int32_t *count, int32_t *index, int batch, int num,
                   float score_threshold, float iou_threshold, int class_aware, int max_out, void *workspace,
                   size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * BEVDet view-transformer index build (csrc/lss_prepare.hip): LSSViewTransformer.get_lidar_coor followed by
 * voxel_pooling_prepare_v2 (third_party/bev_mmdet3d/models/necks/view_transformer.py:126-168, 239-312) on the device,
 * with fixed-size outputs and no host round trip (capturable), so the five index arrays of bev_pool_v2 can follow the
 * calibration of every frame.
 *
 * bevops_lss_voxel_prepare.
 *   frustum [d, h, w, 3] F32 (device): the (u, v, depth) image-plane points of create_frustum.
 *   calib (device, F32, n_cams * 24 + 9 values): per camera [inverse(post_rots) 9 | post_trans 3 | combine 9 | trans 3]
 *   with combine = sensor2ego[:3,:3] @ inverse(cam2imgs) and trans = sensor2ego[:3,3], then bda 9; 3x3 row-major.
 *   The small matrices are the caller's (host) work.
 *   grid_host[9] (host, F32) = lower bound, interval, size of (x, y, z) as create_grid_infos holds them.
 * ARITHMETIC, per frustum point of camera n, F32, every product and sum rounded on its own, each 3x3 . 3x1 product
 *   summed in ascending k ((m0 p0 + m1 p1) + m2 p2), no contraction -- bit-equal to get_lidar_coor on the CPU:
 *   p = frustum - post_trans; p = inverse(post_rots) . p; p = (p.x p.z, p.y p.z, p.z); p = combine . p; p += trans;
 *   coor = bda . p.  coor (NULL or [n_cams, d, h, w, 3] F32) receives these coordinates.
 * CELL: q = (coor - lower) / interval, IEEE division; t = trunc(q), toward zero as `.long()` does (a quotient in
 *   (-1, 0) lands in cell 0); the point is kept when 0 <= t < size on all three axes, tested on the truncated FLOAT, so
 *   a non-finite quotient or one beyond the int32 range drops the point and never becomes an address;
 *   cell = z (ny nx) + y nx + x.
 * ORDER: kept points ascending by cell; inside a cell ascending by point index (the stable sort: a valid reading of
 *   the reference's argsort, whose order among equal keys is unspecified, and the rule that makes the arrays unique).
 *   Intervals are the run-length encoding of the sorted cells.
 * OUTPUTS, int32, fixed capacity: ranks_bev, ranks_depth (= point index ((n d + i) h + j) w + k), ranks_feat
 *   (= (ranks_depth / (d h w)) (h w) + ranks_depth % (h w)): num_points = n_cams d h w entries each; interval_starts,
 *   interval_lengths: min(num_points, cells) entries each; counts[2] = {n_points, n_intervals}.  Entries at and behind
 *   the counts are zero.  No kept point: counts = {0, 0}, all arrays zero, BEVOPS_SUCCESS.
 *   Bit-reproducible: atomics only produce digit counts, never an order.
 * LIMITS, checked before any device call: NULL pointers (coor excepted), non-positive counts, a workspace shorter than
 *   bevops_lss_voxel_prepare_workspace_size(n_cams, d, h, w) or not 16-byte aligned, a non-finite lower bound, a
 *   non-finite or non-positive interval, a size that is non-finite or below 1: BEVOPS_BAD_PARAM.  batch != 1
 *   (the pooling plugin is batch-1), num_points > 4 194 304 (2^22), a non-integral size, cells = nx ny nz >
 *   16 777 216 (2^24): BEVOPS_NOT_SUPPORTED (the workspace size is 0 for such shapes).
 *   Launches: 1 (cells + first digit counts) + 2 or 3 per 8-bit digit of `cells` (two digits up to 65 535 cells) + 4
 *   (run starts, scan, emit, lengths); none sized by a device value.
 *
 * bevops_lss_voxel_prepare_batched: the reference's batched form (get_lidar_coor and voxel_pooling_prepare_v2 carry B
 *   through) for `batch` samples in one call, same kernels, same arithmetic, same stable sort and run-length pass.
 *   calib [batch][n_cams * 24 + 9]: each row is the packed buffer above, so every sample has its own cameras and bda.
 *   Key of a kept point = b * cells + cell (batch * cells for a dropped one); the number of 8-bit passes follows
 *   batch * cells.  OUTPUTS: ranks_bev = b * cells + cell; ranks_depth = the point index over batch n_cams d h w;
 *   ranks_feat = (ranks_depth / (d h w)) (h w) + ranks_depth % (h w) (the reference's index into [B N, h, w]);
 *   num_points = batch n_cams d h w entries each; interval arrays: min(num_points, batch * cells) entries; counts[2] =
 *   the totals over the batch; zero behind the counts; coor NULL or [batch, n_cams, d, h, w, 3].
 *   LIMITS: as above, with num_points <= 2^22 and batch * cells <= 2^24, else BEVOPS_NOT_SUPPORTED (size query 0;
 *   BEVDet-R50 fits up to batch 16); batch <= 0 is BEVOPS_BAD_PARAM.  At batch = 1 every output is bit-identical to
 *   bevops_lss_voxel_prepare's.
 *
 * bevops_bev_pool_v2_forward_indirect: bevops_bev_pool_v2_forward with the interval count read on the device:
 *   n_intervals_dev[0] (clamped to [0, max_intervals]); max_intervals, a host value, sizes the grid and is the
 *   capacity of interval_starts / interval_lengths.  Same kernels and per-interval arithmetic: for equal index arrays
 *   the output is bit-identical to bevops_bev_pool_v2_forward in F32, F16 and I8.  A batch of B grids is this call
 *   with out_height = B * H: the batched ranks_bev already carry b * H * W, so the output is [B, H, W, channels].
 * ------------------------------------------------------------------------ */
size_t bevops_lss_voxel_prepare_workspace_size(int n_cams, int d, int h, int w);
int bevops_lss_voxel_prepare(const float *frustum, const float *calib, const float *grid_host, int32_t *ranks_bev,
                             int32_t *ranks_depth, int32_t *ranks_feat, int32_t *interval_starts,
                             int32_t *interval_lengths, int32_t *counts, float *coor, int batch, int n_cams, int d,
                             int h, int w, void *workspace, size_t workspace_bytes, void *stream);
size_t bevops_lss_voxel_prepare_batched_workspace_size(int batch, int n_cams, int d, int h, int w);
int bevops_lss_voxel_prepare_batched(const float *frustum, const float *calib, const float *grid_host,
                                     int32_t *ranks_bev, int32_t *ranks_depth, int32_t *ranks_feat,
                                     int32_t *interval_starts, int32_t *interval_lengths, int32_t *counts, float *coor,
                                     int batch, int n_cams, int d, int h, int w, void *workspace,
                                     size_t workspace_bytes, void *stream);
int bevops_bev_pool_v2_forward_indirect(int dtype, const void *depth, const void *feat, const int32_t *ranks_depth,
                                        const int32_t *ranks_feat, const int32_t *ranks_bev,
                                        const int32_t *interval_starts, const int32_t *interval_lengths,
                                        const int32_t *n_intervals_dev, void *output, int channels, int max_intervals,
                                        int out_height, int out_width, float scale_depth, float scale_feat,
                                        float scale_out, void *stream);

/* ------------------------------------------------------------------------
 * PTQ calibration on the device (csrc/calibrate.hip, design/calibration.md): a running 2048-bin histogram of |x| per
 * calibration site and the threshold searches over it.  The reference hands calibration to TensorRT
 * (det2trt/quantization/calibrator_trt.py:6-92); these entries are what quantization.py's *_device calibrators call.
 *
 * STATE: bevops_calib_state_size() = 16 448 bytes at a 64-byte aligned address; a zero-filled state is a valid empty
 *   one.  Header (64 bytes): float range (0: no data yet; bin k covers [k, k + 1) range / 2048), float amax (running
 *   maximum of |x|), float batch_amax, uint32 batches, uint64 count (finite elements binned), uint64 nonfinite, uint32
 *   batch_finite, 28 bytes of zero; batch_amax and batch_finite are scratch of one collect call and zero between
 *   calls.  Then uint64 hist[2048].
 *
 * bevops_calib_collect: one batch x[count] (F32 or F16, element-aligned; other dtypes: BEVOPS_NOT_SUPPORTED; count == 0:
 *   BEVOPS_SUCCESS, nothing launched) into `state`.  Three launches, no host read, no allocation: capturable.
 *   1. batch_amax = max |x| over the finite elements (integer atomic max on the bit pattern); NaN and +-inf are
 *      skipped and counted into nonfinite.
 *   2. One block.  A batch without a finite element changes nothing but batches.  Else: range == 0 becomes
 *      max(batch_amax, 1e-12f); while batch_amax > range the range doubles, d times in all, and the bins merge:
 *      new[j] = sum old[j 2^d .. (j + 1) 2^d - 1] for j < 2048 >> d, 0 above (d >= 11: everything in bin 0); amax =
 *      max(amax, batch_amax).  Then batch_amax = 0, batches += 1.
 *   3. bin = min((int)(fl(|x| fl(2048 / range))), 2047) for every finite x, F16 converted to F32 first (exact), both
 *      operations IEEE F32; hist[bin] += 1, count += 1.
 *   Only integer atomics: the state after a call does not depend on the order of arrival and repeats bit for bit.
 *   NULL x / state, a misaligned x or state: BEVOPS_BAD_PARAM.  count > 2^40: BEVOPS_NOT_SUPPORTED.
 *
 * bevops_calib_threshold: bins[s] (int32[num_states]) = the clip bin of state s, the state at states + s state_stride
 *   (state_stride >= the state size, a multiple of 64); -1 for a state with count == 0.  kl (optional,
 *   double[num_states]) receives the minimum of the KL curve for method 0 (+inf where none is finite), 0 for method 1.
 *   method 0, entropy (quantization.py: entropy_threshold_bin on the device): h = hist as double, h[0] = h[1]; for
 *     every i in 128 .. 2048: P = h[:i] with the tail mass added to P[i - 1]; level of bin k =
 *     ((2k + 1) 64 + i - 1) / i - 1 in integers; Q[k] = (sum of its level) / max(non-empty bins of its level, 1)
 *     where h[k] > 0, else 0; KL = sum over pn > 0 of pn log(pn / max(Q / qsum, 1e-12)), pn = P / psum, +inf when
 *     psum <= 0 or qsum <= 0.  bins[s] = (first minimising i) - 1; 2047 when every candidate is infinite.  Sums of
 *     counts are exact; qsum and KL are summed in a fixed order, so results repeat bit for bit.
 *   method 1, percentile: the first k with cdf[k] >= cdf[2047] * percentile / 100.0 (doubles, that operand order),
 *     capped at 2047; no substitution in bin 0.
 *   Other methods: BEVOPS_NOT_SUPPORTED.  NULL states / bins, num_states <= 0, a bad stride or alignment, a negative
 *   or NaN percentile, a workspace that is NULL, not 8-byte aligned or shorter than
 *   bevops_calib_threshold_workspace_size(num_states) (the [num_states, 1921] KL curves; both methods):
 *   BEVOPS_BAD_PARAM.  num_states > 2^20: BEVOPS_NOT_SUPPORTED.  Two launches (method 0) or one (method 1).
 * ------------------------------------------------------------------------ */
size_t bevops_calib_state_size(void);
int bevops_calib_collect(int dtype, const void *x, size_t count, void *state, void *stream);
size_t bevops_calib_threshold_workspace_size(int num_states);
int bevops_calib_threshold(int method, double percentile, const void *states, int num_states, size_t state_stride,
                           int32_t *bins, double *kl, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Grouped, UNMODULATED deformable convolution (DCNv1; csrc/deform_conv.hip, design/bevdepth_dcn.md): the deformable
 * convolution of mmcv's `DCN` pack as BEVDepth's DepthNet places it behind its ASPP block (groups = 4, deform_groups = 1;
 * third_party/bev_mmdet3d/models/necks/view_transformer.py:590-601).  Not a reference plugin.  3 x 3, stride 1,
 * padding 1, dilation 1, ONE deform group, channels-last fp16:
 *   input_nhwc  [B, H, W, Cin], output_nhwc [B, H, W, Cout];
 *   offset_nhwc [B, H, W, offset_channels]: the raw output of the pack's offset convolution (what
 *               bevops_conv3x3_c32_forward_nhwc writes: offset_channels = 32).  Channels [0, 18) are the offsets, (h, w)
 *               per tap, taps row-major; channels >= 18 are never read;
 *   packed_weight: bevops_mdconv_pack_weight(BEVOPS_F16, ...) of weight [Cout, Cin / groups, 3, 3];
 *   bias [Cout] fp16 or NULL; relu 0 or 1.
 * The DCNv2 sampling rules of bevops_mdconv_forward with the mask identically 1: h = y - 1 + i + off_h, w = x - 1 + j +
 * off_w in fp32; a tap contributes iff h > -1 && w > -1 && h < H && w < W; bilinear, corners outside the image
 * contribute zero (and are not read), corners inside are multiplied even by a zero weight; the sample is
 * fma(w11, v11, fma(w10, v10, fma(w01, v01, w00 * v00))) in fp32, rounded once to fp16; fp32 accumulation on the fp16
 * matrix cores over k = (tap, channel); bias and ReLU in fp32; one rounding at the store.
 * One launch for all groups; no workspace, no atomics, no allocation, no synchronisation; capturable.
 * Status, in this order:
 *   BAD_PARAM      a NULL input / offset / weight / output; any pointer (bias included) off a 16-byte boundary; B < 0;
 *                  H, W, Cin, Cout or groups <= 0; relu not 0 / 1; offset_channels < 18 or odd
 *   NOT_SUPPORTED  Cin % groups, Cout % groups, (Cin / groups) % 32 or (Cout / groups) % 32 non-zero;
 *                  B H W > 2^31 - 65 (32-bit pixel index); groups * ceil(Cout / groups / 64) > 65535 (grid rows)
 *   SUCCESS        B == 0, without a launch
 * ------------------------------------------------------------------------ */
int bevops_deform_conv3x3_nhwc_f16(const void *input_nhwc, const void *offset_nhwc, int offset_channels,
                                   const void *packed_weight, const void *bias, void *output_nhwc, int relu,
                                   int B, int H, int W, int Cin, int Cout, int groups, void *stream);

/* ------------------------------------------------------------------------
 * The INT8 form of the convolution above (csrc/deform_conv_s8.hip, design/bevdepth_dcn_int8.md): grouped, unmodulated,
 * deformable, 3 x 3, stride 1, padding 1, dilation 1, ONE deform group, any number of conv groups in ONE launch, on
 * channels-last int8 slices and the int8 matrix cores (v_mfma_i32_32x32x32_i8).  Not a reference plugin.
 *   x_q     int8, real = q scale_a; element (b, y, x, c) at base + ((b H + y) W + x) x_pitch + c, the pitch in elements as
 *           in bevops_conv_slice_s8; x_q and out may be channel slices of wider buffers;
 *   out     int8 (out_dtype BEVOPS_I8, real = q scale_out) or fp16 (BEVOPS_F16), the same addressing with out_pitch;
 *   offset_nhwc_f16 [B, H, W, offset_channels] fp16: the raw rows of the offset convolution, exactly as the fp16 entry
 *           reads them: channels [0, 18) are the offsets, (h, w) per tap, taps row-major; channels >= 18 are never read.
 *           The offsets are NOT quantised;
 *   w_q_taps int8 [Cout][3][3][Cin / groups] (real = q scale_w w_scales[co]): what quantize_weight_taps makes of
 *           [Cout, Cin / groups, 3, 3]; no pack entry, no packed-weight cache;
 *   w_scales fp32 [Cout] or NULL (then 1); bias fp32 [Cout] or NULL; relu 0 or 1.
 * THE ARITHMETIC (every step one fp32 operation):
 *   1. positions  h = (float)(y - 1 + i) + (float)off_h is one fp32 add, w likewise.  A tap is live iff h > -1 && w > -1
 *      && h < H && w < W: a NaN or infinite offset contributes nothing.  lh = h - floorf(h), hh = 1 - lh, likewise for w;
 *      the four corner weights are one fp32 product each, hh hw, hh lw, lh hw, lh lw.  A corner outside the image is not
 *      read and contributes +0.
 *   2. sample     s = w00 * (float)v00; s = fma(w01, (float)v01, s); s = fma(w10, (float)v10, s);
 *      s = fma(w11, (float)v11, s) in fp32; the column byte is c = min(max(rne(s), -127), 127).  The column has the
 *      INPUT's scale (bilinear interpolation is convex): no second scale, no 8-bit area weights -- deliberately not the
 *      DCNv2 plugin's u8 x 255 arithmetic.
 *   3. sum        sum = sum over (tap, ci in group) of c * w_q, exact in int32.
 *   4. epilogue   bevops_conv_slice_s8's order, without an identity: sc = (scale_a * scale_w) * w_scales[co], the product
 *      in parentheses taken on the host; v = fma((float)sum, sc, bias[co]); ReLU if asked for;
 *      int8 out: min(max(rne(v * inv), -127), 127) with inv = 1.f / scale_out taken on the host (a NaN leaves as -127);
 *      fp16 out: one rounding.
 * Byte offsets are 64-bit.  No workspace, no atomics, no allocation, no synchronisation; capturable.
 * Status, in this order:
 *   BAD_PARAM      a NULL x_q / offset / weight / out; any pointer (w_scales and bias included) off a 16-byte boundary;
 *                  B < 0; H, W, Cin, Cout or groups <= 0; relu not 0 / 1; offset_channels < 18 or odd; x_pitch < Cin or
 *                  not a multiple of 16; out_pitch < Cout or not a multiple of 16 (8 for fp16 out); a scale in use
 *                  (scale_a, scale_w; scale_out for int8 out) that is not positive and finite
 *   NOT_SUPPORTED  out_dtype outside {BEVOPS_I8, BEVOPS_F16}; Cin % groups, Cout % groups, (Cin / groups) % 32 or
 *                  (Cout / groups) % 32 non-zero; B H W > 2^31 - 65 (32-bit pixel index);
 *                  groups * ceil(Cout / groups / 64) > 65535 (grid rows)
 *   SUCCESS        B == 0, without a launch
 * ------------------------------------------------------------------------ */
int bevops_deform_conv3x3_nhwc_s8(const void *x_q, int x_pitch, float scale_a, const void *offset_nhwc_f16,
                                  int offset_channels, const void *w_q_taps, const float *w_scales, float scale_w,
                                  const float *bias, int out_dtype, void *out, int out_pitch, float scale_out, int relu,
                                  int B, int H, int W, int Cin, int Cout, int groups, void *stream);
/* BEVStereo's temporal-stereo cost volume (csrc/stereo_cost.hip; DepthNet.gen_grid + calculate_cost_volumn of the
 * reference's view_transformer.py, bevformer_tensorrt_amd/functions/stereo.py) in ONE launch, no workspace, no atomics:
 *   out[n, h, w, :D] = softmax over d of -( sum_c |curr[n,h,w,c] - warp(prev)[n,d,h,w,c]| + bias * [gate == 0] )
 * warp = grid_sample(bilinear, zeros padding, align_corners=True) of prev at grid[n, d, h, w]; gate = the warped value
 * of channel C - 4 (channel 0 of the last group of four), tested for exact equality with zero, skipped when bias == 0.
 * prev, curr: channels-last fp16 [n, Hc, Wc, C] channel slices as in bevops_conv_slice_f16 (pitches in elements, >= C,
 * multiples of 8).  out: channels-last fp16 [n, Hc, Wc, Dpad] slice (out_pitch >= Dpad), columns D .. Dpad written as
 * exact zeros.  The blend, the sum and the softmax run in fp32 in the fixed order csrc/stereo_cost.hip states; ONE
 * rounding.  A corner outside the image counts as zero and is not read; a NaN or infinite grid value is outside.
 * grid != NULL: fp32 [n, D, Hc, Wc, 2], normalised (x, y) as gen_grid returns it.  grid == NULL: the kernel computes
 * the same values from consts (fp32, 40 floats per camera: inverse(post_rots) 9 | post_trans 3 | k2s_R @ inverse(K) 9 |
 * k2s_t 3 | K 9 | post_rots[:2,:2] 4 | post_trans[:2] 2 | pad 1) and the frustum tables xs[Wc], ys[Hc], ds[D] (the
 * values of create_frustum(..., downsample=4)): the reference's fp32 op sequence, every product, sum and quotient
 * rounded on its own, points with z < 1e-3 sent to (-2, -2), normalised by the image size (4 Hc, 4 Wc).
 * bevops_stereo_grid writes exactly those values as fp32 [n, D, Hc, Wc, 2]; the fused entry with grid == NULL equals
 * itself fed with that grid bit for bit.
 * Statuses, in this order (bevops_conv_slice_f16's): NULL prev / curr / out, n < 0, non-positive Hc / Wc / C / D / Dpad;
 * grid == NULL with a NULL consts / xs / ys / ds; a pitch below its channel count, Dpad < D; a pitch that is no
 * multiple of 8; prev / curr / out not 16-byte aligned, grid not 8-byte, a table not 4-byte aligned; a NaN bias:
 * BEVOPS_BAD_PARAM.  C % 8 != 0 (the reference silently drops C % 4 trailing channels; this entry refuses), D > 128,
 * Dpad % 8 != 0, n Hc Wc > 0x3fffffff, Hc or Wc above 0xffffff: BEVOPS_NOT_SUPPORTED.  n == 0: BEVOPS_SUCCESS without a
 * launch.  bevops_stereo_grid: NULL operands, n < 0, non-positive D / Hc / Wc, misaligned pointers: BEVOPS_BAD_PARAM;
 * D > 128 and the same size limits: BEVOPS_NOT_SUPPORTED. */
int bevops_stereo_grid(const float *consts, const float *xs, const float *ys, const float *ds, float *grid, int n, int D,
                       int Hc, int Wc, void *stream);
int bevops_stereo_cost_volume_f16(const void *prev, int prev_pitch, const void *curr, int curr_pitch, const float *grid,
                                  const float *consts, const float *xs, const float *ys, const float *ds, void *out,
                                  int out_pitch, int n, int Hc, int Wc, int C, int D, int Dpad, float bias, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BEVOPS_H_ */
