"""Operator API: same names and positional signatures as the reference's
det2trt/models/functions/__init__.py:1-35, registered in TRT_FUNCTIONS."""
from .multi_scale_deformable_attn import (
    multi_scale_deformable_attn,
    multi_scale_deformable_attn2,
    multi_scale_deformable_attn_int8,
    multi_scale_deformable_attn_local,
    msda_pack_value,
    multi_scale_deformable_attn_prepacked,
)
from .rotate import rotate, rotate2, rotate_int8, rotate_hwc
from .grid_sampler import grid_sampler, grid_sampler2, grid_sampler_int8
from .bev_pool_v2 import bev_pool_v2, bev_pool_v2_2, bev_pool_v2_int8
from .modulated_deformable_conv2d import (modulated_deformable_conv2d, modulated_deformable_conv2d2,
                                          modulated_deformable_conv2d_int8, modulated_deformable_conv2d_nhwc,
                                          bias_act_nhwc_, bias_relu_maxpool_nhwc, conv_offset_nhwc, upsample_add_nhwc_,
                                          feat_embed_nhwc)
from .spatial_cross_attention import (spatial_cross_attention_sample, spatial_cross_attention_projected,
                                      spatial_cross_attention_plan)
from .linear import (linear_bias_act, layer_norm, quantize_rows, dequantize_rows, linear_int8, tsgemm, tsgemm_ln, tsgemm_grouped, tile_gemm, tile_gemm_dst, gemm2, small_gemm, small_gemm_dst,
                     dense_auto, tsa_split, queue_mean2, row_chain, pack_chain_weight)
from .int8_chain import linear_int8_chain, linear_int8_ln, conv_int8_chain_nhwc, modulated_deformable_conv2d_int8_nhwc
from .conv import conv_nhwc, conv3x3_nhwc, conv3x3_auto, conv3x3_c64, conv_int8_nhwc, stem_conv_pool
from .image import (image_normalize_pad, padded_size, bevdet_test_augmentation, bevdet_post_transform, image_resize_plan,
                    image_resize_crop_normalize, BEVFORMER_IMAGE_PIPELINES, scaled_size, scale_lidar2img,
                    image_normalize_resize_pad, DETECT2D_IMAGE_PIPELINES, keep_ratio_size, yolox_test_geometry,
                    centernet_test_geometry, image_letterbox)
from .point_sampling import point_sampling
from .attention import self_attention_qkv
from .refine import refine_reference_points, decode_boxes
from .multi_head_attn import qkv, qkv2
from .inverse import inverse
from .decode import nms_free_decode, centerpoint_decode
from .nms import bev_nms, nms_bev, circle_nms, bev_iou
from .decode2d import centernet_decode, yolox_decode, box_nms
from .lss_prepare import (lss_voxel_prepare, lss_lidar_coor, bev_pool_v2_indirect, lss_voxel_prepare_batched,
                          lss_lidar_coor_batched)
from .calibrate import calib_state_size, calib_collect, calib_threshold
from .bev_half import lss_depth_split, upsample_bilinear_concat_nhwc, lss_depth_split_q, upsample_bilinear_nhwc_q
from .deconv import conv_transpose2d_nhwc, pack_deconv4x4s2, deconv_packed_weight, conv_transpose2d_q_nhwc, quantize_deconv_weight
from .yolox_ops import (conv_slice_nhwc, conv_slice_taps, conv_slice_packed_weight, focus_nhwc, spp_maxpool_nhwc,
                        upsample_nearest2x_nhwc, pad_channels, unpad_channels, conv_slice_q_taps, focus_nhwc_q,
                        quantize_weight_taps)
from .lss_depthnet import (lss_camera_gate, se_gate2_nhwc, global_avgpool_nhwc, pack_camera_gate, camera_gate_packed,
                           se_gate2_nhwc_q, global_avgpool_nhwc_q)
from .deform_conv import deform_conv2d, deform_conv2d_nhwc, deform_conv2d_q_nhwc, deform_conv_packed_weight
from .stereo import (stereo_calibration, stereo_frustum_tables, stereo_grid, stereo_grid_plain, stereo_cost_volume,
                     stereo_cost_volume_plain)
from ..utils.register import TRT_FUNCTIONS

TRT_FUNCTIONS.register_module(module=multi_scale_deformable_attn)
TRT_FUNCTIONS.register_module(module=multi_scale_deformable_attn2)
TRT_FUNCTIONS.register_module(module=multi_scale_deformable_attn_int8)
for _f in (rotate, rotate2, rotate_int8, grid_sampler, grid_sampler2, grid_sampler_int8,
           bev_pool_v2, bev_pool_v2_2, bev_pool_v2_int8, modulated_deformable_conv2d,
           modulated_deformable_conv2d2, modulated_deformable_conv2d_int8,
           spatial_cross_attention_sample, inverse, qkv, qkv2):
    TRT_FUNCTIONS.register_module(module=_f)

__all__ = [
    "multi_scale_deformable_attn",
    "multi_scale_deformable_attn2",
    "multi_scale_deformable_attn_int8",
    "rotate", "rotate2", "rotate_int8",
    "grid_sampler", "grid_sampler2", "grid_sampler_int8",
    "bev_pool_v2", "bev_pool_v2_2", "bev_pool_v2_int8",
    "modulated_deformable_conv2d", "modulated_deformable_conv2d2", "modulated_deformable_conv2d_int8",
    "inverse", "qkv", "qkv2",
    "nms_free_decode", "centerpoint_decode",
    "bev_nms", "nms_bev", "circle_nms", "bev_iou",
    "centernet_decode", "yolox_decode", "box_nms",
    "lss_voxel_prepare", "lss_lidar_coor", "bev_pool_v2_indirect", "lss_voxel_prepare_batched", "lss_lidar_coor_batched",
    "calib_state_size", "calib_collect", "calib_threshold",
    "bevdet_test_augmentation", "bevdet_post_transform", "image_resize_plan", "image_resize_crop_normalize",
    "BEVFORMER_IMAGE_PIPELINES", "scaled_size", "scale_lidar2img", "image_normalize_resize_pad",
    "DETECT2D_IMAGE_PIPELINES", "keep_ratio_size", "yolox_test_geometry", "centernet_test_geometry", "image_letterbox",
    "spatial_cross_attention_sample", "spatial_cross_attention_projected", "spatial_cross_attention_plan", "modulated_deformable_conv2d_nhwc", "bias_act_nhwc_", "linear_bias_act", "layer_norm", "rotate_hwc", "conv_offset_nhwc", "upsample_add_nhwc_", "feat_embed_nhwc",
    "msda_pack_value", "multi_scale_deformable_attn_prepacked", "multi_scale_deformable_attn_local", "image_normalize_pad", "padded_size", "quantize_rows", "dequantize_rows", "linear_int8", "tsgemm", "tsgemm_ln", "tsgemm_grouped", "tile_gemm", "tile_gemm_dst", "gemm2", "small_gemm_dst", "small_gemm", "row_chain", "pack_chain_weight", "dense_auto", "tsa_split", "queue_mean2", "conv_nhwc", "conv3x3_nhwc", "conv3x3_auto", "conv3x3_c64", "conv_int8_nhwc", "bias_relu_maxpool_nhwc", "stem_conv_pool", "point_sampling", "self_attention_qkv", "refine_reference_points", "decode_boxes",
    "linear_int8_chain", "linear_int8_ln", "conv_int8_chain_nhwc", "modulated_deformable_conv2d_int8_nhwc",
    "lss_depth_split", "upsample_bilinear_concat_nhwc", "lss_depth_split_q", "upsample_bilinear_nhwc_q",
    "conv_transpose2d_nhwc", "pack_deconv4x4s2", "deconv_packed_weight", "conv_transpose2d_q_nhwc", "quantize_deconv_weight",
    "conv_slice_nhwc", "conv_slice_taps", "conv_slice_packed_weight", "focus_nhwc", "spp_maxpool_nhwc",
    "upsample_nearest2x_nhwc", "pad_channels", "unpad_channels",
    "conv_slice_q_taps", "focus_nhwc_q", "quantize_weight_taps",
    "lss_camera_gate", "se_gate2_nhwc", "global_avgpool_nhwc", "pack_camera_gate", "camera_gate_packed",
    "se_gate2_nhwc_q", "global_avgpool_nhwc_q",
    "deform_conv2d", "deform_conv2d_nhwc", "deform_conv2d_q_nhwc", "deform_conv_packed_weight",
    "stereo_calibration", "stereo_frustum_tables", "stereo_grid", "stereo_grid_plain", "stereo_cost_volume",
    "stereo_cost_volume_plain",
]
