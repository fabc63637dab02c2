"""The BEVDet view transformer's index build on the device (csrc/lss_prepare.hip): get_lidar_coor +
voxel_pooling_prepare_v2 of third_party/bev_mmdet3d/models/necks/view_transformer.py:126-168, 239-312 as HIP launches
with fixed-size outputs, and bev_pool_v2 with the interval count read from the device.  None of these is a function of
the reference's registry (the reference evaluates the ranks with host-side torch code and feeds them to the engine,
tools/bevdet/evaluate_trt.py:107-127), so TRT_FUNCTIONS does not list them.

`calib` is the packed fp32 buffer of LSSViewTransformer.calibration_matrices: per camera
[inverse(post_rots) 9 | post_trans 3 | combine 9 | trans 3], then bda 9.  The `_batched` calls take one such row per sample,
calib [B, n_cams * 24 + 9] (LSSViewTransformer.calibration_matrices_batched), and return the reference's batched arrays:
ranks_bev = b * cells + cell, ranks_depth / ranks_feat over B * n_cams cameras."""
import ctypes

import torch

from ..utils import lib as _lib

CALIB_PER_CAMERA, CALIB_TAIL = 24, 9


def calib_cameras(calib):
    n, r = divmod(calib.numel() - CALIB_TAIL, CALIB_PER_CAMERA)
    if n < 1 or r:
        raise ValueError(f"calib holds {calib.numel()} values; expected n_cams * {CALIB_PER_CAMERA} + {CALIB_TAIL}")
    return n


def _grid9(grid_lower_bound, grid_interval, grid_size):
    vals = [float(v) for t in (grid_lower_bound, grid_interval, grid_size) for v in torch.as_tensor(t, dtype=torch.float32)]
    if len(vals) != 9:
        raise ValueError("grid_lower_bound, grid_interval and grid_size hold three values each")
    return (ctypes.c_float * 9)(*vals), vals


def _prepare(frustum, calib, grid_lower_bound, grid_interval, grid_size, want_coor, batched=False):
    assert frustum.is_cuda and calib.is_cuda, "lss_voxel_prepare: frustum / calib must be on the GPU"
    if frustum.dtype != torch.float32 or calib.dtype != torch.float32:
        raise TypeError("lss_voxel_prepare: frustum and calib are float32")
    if frustum.dim() != 4 or frustum.shape[-1] != 3:
        raise ValueError(f"frustum is [D, H, W, 3], got {tuple(frustum.shape)}")
    handle = _lib.load_library()
    dev = frustum.device
    if batched:
        if calib.dim() != 2 or calib.shape[0] < 1:
            raise ValueError(f"calib is [B, n_cams * {CALIB_PER_CAMERA} + {CALIB_TAIL}], got {tuple(calib.shape)}")
        batch = calib.shape[0]
        frustum, calib = frustum.contiguous(), calib.contiguous()
        n = calib_cameras(calib[0])
    else:
        batch = 1
        frustum, calib = frustum.contiguous(), calib.contiguous().view(-1)
        n = calib_cameras(calib)
    d, h, w, _ = frustum.shape
    grid, vals = _grid9(grid_lower_bound, grid_interval, grid_size)
    num_points = batch * n * d * h * w
    cells = batch * vals[6] * vals[7] * vals[8]
    cap = int(min(num_points, cells)) if cells == cells and cells >= 1 else 1
    i32 = dict(dtype=torch.int32, device=dev)
    rb, rd, rf = (torch.empty(num_points, **i32) for _ in range(3))
    ist, il = torch.empty(cap, **i32), torch.empty(cap, **i32)
    counts = torch.empty(2, **i32)
    coor = torch.empty(batch, n, d, h, w, 3, dtype=torch.float32, device=dev) if want_coor else None
    if batched:
        name, entry = "bevops_lss_voxel_prepare_batched", handle.bevops_lss_voxel_prepare_batched
        ws_bytes = handle.bevops_lss_voxel_prepare_batched_workspace_size(batch, n, d, h, w)
    else:
        name, entry = "bevops_lss_voxel_prepare", handle.bevops_lss_voxel_prepare
        ws_bytes = handle.bevops_lss_voxel_prepare_workspace_size(n, d, h, w)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        st = entry(
            frustum.data_ptr(), calib.data_ptr(), ctypes.cast(grid, ctypes.c_void_p), rb.data_ptr(), rd.data_ptr(),
            rf.data_ptr(), ist.data_ptr(), il.data_ptr(), counts.data_ptr(), coor.data_ptr() if want_coor else None,
            batch, n, d, h, w, ws.data_ptr(), ws_bytes, _lib.current_stream_ptr(dev))
    _lib.check(st, name)
    return (rb, rd, rf, ist, il, counts), coor


def lss_voxel_prepare(frustum, calib, grid_lower_bound, grid_interval, grid_size, padded=True):
    """LSSViewTransformer.get_bev_pool_input on the device.  frustum [D, H, W, 3] fp32 and calib (packed, see the
    module docstring) on the GPU; the grid triple as create_grid_infos holds it (host values).
    padded=True: (ranks_bev, ranks_depth, ranks_feat [N D H W], interval_starts, interval_lengths [min(points, cells)],
    counts [2] = {n_points, n_intervals}), int32, zero behind the counts, no host synchronisation (capturable).
    padded=False: the counts are read once and the five tensors come back trimmed, in the reference's form and argument
    order -- or five None when no point is kept, as the reference returns.  Inside a cell the points are in ascending
    point index (the stable order; the reference's argsort leaves it unspecified)."""
    return _trimmed(_prepare(frustum, calib, grid_lower_bound, grid_interval, grid_size, False)[0], padded)


def _trimmed(out, padded):
    if padded:
        return out
    n_pts, n_int = out[5].tolist()
    if n_int == 0:
        return None, None, None, None, None
    return out[0][:n_pts], out[1][:n_pts], out[2][:n_pts], out[3][:n_int], out[4][:n_int]


def lss_voxel_prepare_batched(frustum, calib, grid_lower_bound, grid_interval, grid_size, padded=True):
    """`lss_voxel_prepare` for B samples in one call: calib [B, n_cams * 24 + 9], one packed row per sample (its own
    cameras and bda).  The reference's batched arrays: ranks_bev = b * cells + cell, ranks_depth the point index over
    B N D H W, ranks_feat the index into [B N, H, W]; interval arrays of capacity min(points, B * cells); counts [2] =
    the totals over the batch.  Same kernels and order rule; at B = 1 bit-identical to `lss_voxel_prepare`.
    B N D H W <= 2^22 and B * cells <= 2^24."""
    return _trimmed(_prepare(frustum, calib, grid_lower_bound, grid_interval, grid_size, False, batched=True)[0], padded)


def lss_lidar_coor_batched(frustum, calib, grid_lower_bound, grid_interval, grid_size):
    """The lidar-frame coordinates [B, N, D, H, W, 3] fp32 of the batched index build (calib [B, n_cams * 24 + 9])."""
    return _prepare(frustum, calib, grid_lower_bound, grid_interval, grid_size, True, batched=True)[1]


def lss_lidar_coor(frustum, calib, grid_lower_bound, grid_interval, grid_size):
    """The lidar-frame coordinates [1, N, D, H, W, 3] fp32 of the frustum points as the index build evaluates them:
    bit-equal to LSSViewTransformer.get_lidar_coor on the CPU."""
    return _prepare(frustum, calib, grid_lower_bound, grid_interval, grid_size, True)[1]


def bev_pool_v2_indirect(depth, feat, ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths, counts,
                         out_height=128, out_width=128, scales=None, batch=1):
    """bev_pool_v2 (any of its three flavours, by dtype; int8 takes scales = (depth, feat, out)) on the PADDED arrays
    of lss_voxel_prepare: the interval count is counts[1], read on the device; the capacity of interval_starts sizes
    the launch.  Bit-identical to bev_pool_v2 on the trimmed arrays.  batch = B with the arrays of
    lss_voxel_prepare_batched (depth / feat over B * n_cams cameras) returns [B, out_height, out_width, C]: the same C
    entry with out_height = B * out_height, since the batched ranks_bev carry b * out_height * out_width."""
    assert depth.is_cuda and feat.is_cuda, "bev_pool_v2_indirect: depth/feat must be on the GPU"
    if depth.dtype != feat.dtype:
        raise TypeError(f"depth dtype {depth.dtype} != feat dtype {feat.dtype}")
    if feat.dtype == torch.int8 and scales is None:
        raise ValueError("int8 pooling needs scales = (scale_depth, scale_feat, scale_out)")
    handle = _lib.load_library()
    dev = feat.device
    depth, feat = depth.contiguous(), feat.contiguous()
    for t in (ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths, counts):
        if t.dtype != torch.int32 or t.device != dev or not t.is_contiguous():
            raise TypeError("bev_pool_v2_indirect takes the contiguous int32 device arrays of lss_voxel_prepare")
    if counts.numel() != 2 or interval_lengths.numel() != interval_starts.numel():
        raise ValueError("counts holds {n_points, n_intervals}; interval_starts / interval_lengths share one capacity")
    scales = scales or (1.0, 1.0, 1.0)
    c = feat.shape[-1]
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"bev_pool_v2_indirect: batch = {batch}")
    out = torch.empty((batch, out_height, out_width, c), dtype=feat.dtype, device=dev)
    with torch.cuda.device(dev):
        st = handle.bevops_bev_pool_v2_forward_indirect(
            _lib.torch_dtype_code(feat), depth.data_ptr(), feat.data_ptr(), ranks_depth.data_ptr(),
            ranks_feat.data_ptr(), ranks_bev.data_ptr(), interval_starts.data_ptr(), interval_lengths.data_ptr(),
            counts.data_ptr() + 4, out.data_ptr(), c, interval_starts.numel(), batch * out_height, out_width,
            float(scales[0]), float(scales[1]), float(scales[2]), _lib.current_stream_ptr(dev))
    _lib.check(st, "bevops_bev_pool_v2_forward_indirect")
    return out
