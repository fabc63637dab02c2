"""Glue of BEVDet's BEV half on channels-last fp16 activations (csrc/lss_split.hip).  Neither operator is one of the
reference's registry functions (TensorRT owns these layers there), so neither is in TRT_FUNCTIONS.

`lss_depth_split`: depth_net's pixel rows -> the two operands of bev_pool_v2 (softmax over the depth bins, plane-major;
the context features, pixel-major) in one launch.  `upsample_bilinear_concat_nhwc`: FPN_LSS's
`cat([a, interpolate(b, bilinear, align_corners=True)], 1)` in one launch without the up-sampled intermediate.

Both check their arguments before the C ABI is reached: a wrong type or dtype raises TypeError, a shape or layout outside
the entry's domain ValueError, a tensor that is not on the GPU TypeError (checked last, so the domain checks can be
exercised without a device)."""
import numbers

import torch

from ..utils import lib as _lib


def _fp16(t, what):
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float16:
        raise TypeError(f"{what} must be float16, got {t.dtype}")


def _on_gpu(t, what):
    if not t.is_cuda:
        raise TypeError(f"{what} must be on the GPU, got a {t.device.type} tensor")


def lss_depth_split(x, n, D, C, depth_offset, feat_offset=0, spatial=None):
    """x [n * hw, row_stride] fp16 rows (contiguous) with the depth logits in columns depth_offset .. + D and the
    features in feat_offset .. + C  ->  (depth, feat): depth [n, D, hw] = softmax over each pixel's D logits (fp32
    exponentials and sum, one division, one rounding), feat [n, hw, C] = the feature columns bit for bit.
    spatial=(H, W) with H * W == hw returns them as [n, D, H, W] and [n, H, W, C], the shapes bev_pool_v2 takes.
    1 <= D <= 256; C, feat_offset and row_stride multiples of 8; the two column ranges inside the row and disjoint."""
    _fp16(x, "lss_depth_split: x")
    n, D, C, depth_offset, feat_offset = int(n), int(D), int(C), int(depth_offset), int(feat_offset)
    if x.dim() != 2 or not x.is_contiguous():
        raise ValueError(f"lss_depth_split: x must be contiguous [rows, row_stride], got {tuple(x.shape)} / {x.stride()}")
    rows, stride = x.shape
    if n < 0 or (n == 0 and rows != 0) or (n > 0 and rows % n != 0):
        raise ValueError(f"lss_depth_split: {rows} rows do not split into n = {n} images")
    hw = rows // n if n > 0 else 0
    if not 1 <= D <= 256:
        raise ValueError(f"lss_depth_split: D = {D} outside 1 .. 256")
    if C <= 0 or C % 8 or feat_offset % 8 or stride % 8:
        raise ValueError(f"lss_depth_split: C = {C}, feat_offset = {feat_offset} and row_stride = {stride} must be "
                         "multiples of 8 (C > 0)")
    if depth_offset < 0 or feat_offset < 0 or depth_offset + D > stride or feat_offset + C > stride:
        raise ValueError("lss_depth_split: a column range leaves the row")
    if not (depth_offset + D <= feat_offset or feat_offset + C <= depth_offset):
        raise ValueError("lss_depth_split: the depth and feature columns overlap")
    if spatial is not None and int(spatial[0]) * int(spatial[1]) != hw:
        raise ValueError(f"lss_depth_split: spatial = {tuple(spatial)} does not match {hw} pixels per image")
    _on_gpu(x, "lss_depth_split: x")
    if spatial is not None:
        H, W = int(spatial[0]), int(spatial[1])
        depth = torch.empty((n, D, H, W), dtype=x.dtype, device=x.device)
        feat = torch.empty((n, H, W, C), dtype=x.dtype, device=x.device)
    else:
        depth = torch.empty((n, D, hw), dtype=x.dtype, device=x.device)
        feat = torch.empty((n, hw, C), dtype=x.dtype, device=x.device)
    if rows == 0:
        return depth, feat
    handle = _lib.load_library()
    with torch.cuda.device(x.device):
        st = handle.bevops_lss_depth_split(_lib.F16, x.data_ptr(), depth.data_ptr(), feat.data_ptr(), n, hw, stride,
                                           depth_offset, D, feat_offset, C, _lib.current_stream_ptr(x.device))
    _lib.check(st, "bevops_lss_depth_split")
    return depth, feat


def upsample_bilinear_concat_nhwc(a, b, size=None, scale_factor=None):
    """cat([a, F.interpolate(b, size, mode="bilinear", align_corners=True)], 1) on channels-last fp16 [N, C, H, W]
    tensors in one launch; the result is channels-last.  a = None: the plain up-sampling, to `size` = (h, w) or by the
    integer `scale_factor`; with `a` the output takes a's spatial size.  Four corners weighted in fp32, one rounding.
    Channel counts are multiples of 8."""
    _fp16(b, "upsample_bilinear_concat_nhwc: b")
    if b.dim() != 4 or not b.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("upsample_bilinear_concat_nhwc: b must be a channels-last [N, C, H, W] tensor")
    n, cb, hb, wb = b.shape
    if a is not None:
        _fp16(a, "upsample_bilinear_concat_nhwc: a")
        if a.device != b.device:
            raise TypeError("upsample_bilinear_concat_nhwc: a and b are on different devices")
        if a.dim() != 4 or not a.is_contiguous(memory_format=torch.channels_last) or a.shape[0] != n:
            raise ValueError("upsample_bilinear_concat_nhwc: a must be a channels-last [N, C, H, W] tensor of b's batch")
        ca, h, w = a.shape[1], a.shape[2], a.shape[3]
        if size is not None and (int(size[0]), int(size[1])) != (h, w):
            raise ValueError(f"upsample_bilinear_concat_nhwc: size = {tuple(size)} differs from a's {(h, w)}")
    else:
        ca = 0
        if size is not None:
            h, w = int(size[0]), int(size[1])
        elif scale_factor is not None:
            if int(scale_factor) != scale_factor or scale_factor < 1:
                raise ValueError("upsample_bilinear_concat_nhwc: scale_factor must be a positive integer")
            h, w = hb * int(scale_factor), wb * int(scale_factor)
        else:
            raise ValueError("upsample_bilinear_concat_nhwc: without `a`, give size or scale_factor")
    if ca % 8 or cb % 8 or cb == 0:
        raise ValueError(f"upsample_bilinear_concat_nhwc: channel counts {ca}, {cb} must be multiples of 8")
    if min(h, w, hb, wb) < 1:
        raise ValueError("upsample_bilinear_concat_nhwc: empty image")
    _on_gpu(b, "upsample_bilinear_concat_nhwc: b")
    out = torch.empty((n, ca + cb, h, w), dtype=b.dtype, device=b.device, memory_format=torch.channels_last)
    if n == 0:
        return out
    handle = _lib.load_library()
    with torch.cuda.device(b.device):
        st = handle.bevops_upsample_bilinear_concat_nhwc(_lib.F16, a.data_ptr() if ca else None, b.data_ptr(),
                                                         out.data_ptr(), n, h, w, ca, hb, wb, cb,
                                                         _lib.current_stream_ptr(b.device))
    _lib.check(st, "bevops_upsample_bilinear_concat_nhwc")
    return out


# ---- the INT8 siblings (csrc/lss_split_s8.hip; the BEV half of the INT8 build of BEVDet).  A tensor carries no scale:
# the caller passes it.

def _int8(t, what):
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.int8:
        raise TypeError(f"{what} must be int8, got {t.dtype}")


def _scale(v, what):
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise TypeError(f"{what} must be a number, got {type(v).__name__}")
    v = float(v)
    if not (0.0 < v < float("inf")) or not (0.0 < torch.tensor(v, dtype=torch.float32).item() < float("inf")):
        raise ValueError(f"{what} must be positive and finite in fp32, got {v}")
    return v


def lss_depth_split_q(x, n, D, C, depth_offset, feat_offset, scale_depth, scale_feat, spatial=None):
    """`lss_depth_split` leaving as the INT8 operands of bev_pool_v2 (bevops_lss_depth_split_s8): x [n * hw,
    row_stride] fp16 rows -> (depth_q int8 [n, D, hw], feat_q int8 [n, hw, C]), depth_q = clamp(rne(softmax /
    scale_depth), -127, 127), feat_q = clamp(rne(x / scale_feat), -127, 127); include/bevops.h states the operation
    order.  spatial=(H, W) returns [n, D, H, W] and [n, H, W, C].  1 <= D <= 256; C a multiple of 16; feat_offset and
    row_stride multiples of 8; the two column ranges inside the row and disjoint; scales positive and finite."""
    _fp16(x, "lss_depth_split_q: x")
    sd, sf = _scale(scale_depth, "lss_depth_split_q: scale_depth"), _scale(scale_feat, "lss_depth_split_q: scale_feat")
    n, D, C, depth_offset, feat_offset = int(n), int(D), int(C), int(depth_offset), int(feat_offset)
    if x.dim() != 2 or not x.is_contiguous():
        raise ValueError(f"lss_depth_split_q: x must be contiguous [rows, row_stride], got {tuple(x.shape)} / {x.stride()}")
    rows, stride = x.shape
    if n < 0 or (n == 0 and rows != 0) or (n > 0 and rows % n != 0):
        raise ValueError(f"lss_depth_split_q: {rows} rows do not split into n = {n} images")
    hw = rows // n if n > 0 else 0
    if not 1 <= D <= 256:
        raise ValueError(f"lss_depth_split_q: D = {D} outside 1 .. 256")
    if C <= 0 or C % 16 or feat_offset % 8 or stride % 8:
        raise ValueError(f"lss_depth_split_q: C = {C} must be a positive multiple of 16, feat_offset = {feat_offset} and "
                         f"row_stride = {stride} multiples of 8")
    if depth_offset < 0 or feat_offset < 0 or depth_offset + D > stride or feat_offset + C > stride:
        raise ValueError("lss_depth_split_q: a column range leaves the row")
    if not (depth_offset + D <= feat_offset or feat_offset + C <= depth_offset):
        raise ValueError("lss_depth_split_q: the depth and feature columns overlap")
    if spatial is not None and int(spatial[0]) * int(spatial[1]) != hw:
        raise ValueError(f"lss_depth_split_q: spatial = {tuple(spatial)} does not match {hw} pixels per image")
    _on_gpu(x, "lss_depth_split_q: x")
    if spatial is not None:
        H, W = int(spatial[0]), int(spatial[1])
        depth = torch.empty((n, D, H, W), dtype=torch.int8, device=x.device)
        feat = torch.empty((n, H, W, C), dtype=torch.int8, device=x.device)
    else:
        depth = torch.empty((n, D, hw), dtype=torch.int8, device=x.device)
        feat = torch.empty((n, hw, C), dtype=torch.int8, device=x.device)
    if rows == 0:
        return depth, feat
    handle = _lib.load_library()
    with torch.cuda.device(x.device):
        st = handle.bevops_lss_depth_split_s8(x.data_ptr(), depth.data_ptr(), feat.data_ptr(), n, hw, stride, depth_offset,
                                              D, feat_offset, C, sd, sf, _lib.current_stream_ptr(x.device))
    _lib.check(st, "bevops_lss_depth_split_s8")
    return depth, feat


def _slice_pitch_s8(t, what):
    """Pitch in elements of an int8 channel slice [N, C, H, W] of a channels-last tensor; ValueError for another layout."""
    if t.dim() != 4:
        raise ValueError(f"{what} must be a [N, C, H, W] channel slice of a channels-last tensor")
    N, C, H, W = t.shape
    if W > 1:
        pitch = t.stride(3)
    elif H > 1:
        pitch = t.stride(2)
    elif N > 1:
        pitch = t.stride(0)
    else:
        pitch = (C + 15) // 16 * 16
    ok = pitch >= C and (C == 1 or t.stride(1) == 1) and (W == 1 or t.stride(3) == pitch) and \
        (H == 1 or t.stride(2) == W * pitch) and (N == 1 or t.stride(0) == H * W * pitch)
    if not ok:
        raise ValueError(f"{what} is not a channel slice of a channels-last tensor (shape {tuple(t.shape)}, strides "
                         f"{tuple(t.stride())})")
    if pitch % 16 or (t.storage_offset() % 16 if not t.is_cuda else t.data_ptr() % 16):
        raise ValueError(f"{what}: an int8 slice starts on a 16-byte boundary and its pitch is a multiple of 16 "
                         f"(pitch {pitch})")
    return pitch


def upsample_bilinear_nhwc_q(b_q, scale_b, scale_out, size=None, scale_factor=None, out=None):
    """F.interpolate(b, size, mode="bilinear", align_corners=True) on the int8 channel slice b_q [N, C, hb, wb] (real =
    q scale_b) of a channels-last tensor, requantised with scale_out (bevops_upsample_bilinear_s8; include/bevops.h
    states the operation order).  To `size` = (h, w), by the integer `scale_factor`, or into `out`, an int8 channel slice
    [N, C, h, w] of the consumer's buffer (FPN_LSS's concatenation: the other channels' producer writes its own slice).
    Without `out` the result is a new channels-last tensor.  C a multiple of 16; b_q must not overlap out."""
    _int8(b_q, "upsample_bilinear_nhwc_q: b_q")
    sb, so = _scale(scale_b, "upsample_bilinear_nhwc_q: scale_b"), _scale(scale_out, "upsample_bilinear_nhwc_q: scale_out")
    if out is not None:
        _int8(out, "upsample_bilinear_nhwc_q: out")
        if out.device != b_q.device:
            raise TypeError("upsample_bilinear_nhwc_q: b_q and out are on different devices")
    if b_q.dim() != 4:
        raise ValueError("upsample_bilinear_nhwc_q: b_q must be a [N, C, H, W] channel slice of a channels-last tensor")
    n, C, hb, wb = b_q.shape
    if out is not None:
        if out.dim() != 4 or out.shape[0] != n or out.shape[1] != C:
            raise ValueError(f"upsample_bilinear_nhwc_q: out must be [{n}, {C}, h, w], got {tuple(out.shape)}")
        h, w = out.shape[2], out.shape[3]
        if size is not None and (int(size[0]), int(size[1])) != (h, w):
            raise ValueError(f"upsample_bilinear_nhwc_q: size = {tuple(size)} differs from out's {(h, w)}")
    elif size is not None:
        h, w = int(size[0]), int(size[1])
    elif scale_factor is not None:
        if int(scale_factor) != scale_factor or scale_factor < 1:
            raise ValueError("upsample_bilinear_nhwc_q: scale_factor must be a positive integer")
        h, w = hb * int(scale_factor), wb * int(scale_factor)
    else:
        raise ValueError("upsample_bilinear_nhwc_q: give size, scale_factor or out")
    if C == 0 or C % 16:
        raise ValueError(f"upsample_bilinear_nhwc_q: the channel count {C} must be a positive multiple of 16")
    if min(h, w, hb, wb) < 1:
        raise ValueError("upsample_bilinear_nhwc_q: empty image")
    if h * hb >= 2 ** 31 or w * wb >= 2 ** 31:
        raise ValueError("upsample_bilinear_nhwc_q: h * hb and w * wb must stay below 2^31")
    bp = _slice_pitch_s8(b_q, "upsample_bilinear_nhwc_q: b_q")
    op = _slice_pitch_s8(out, "upsample_bilinear_nhwc_q: out") if out is not None else C
    _on_gpu(b_q, "upsample_bilinear_nhwc_q: b_q")
    if out is None:
        out = torch.empty((n, h, w, C), dtype=torch.int8, device=b_q.device).permute(0, 3, 1, 2)
    if n == 0:
        return out
    handle = _lib.load_library()
    with torch.cuda.device(b_q.device):
        st = handle.bevops_upsample_bilinear_s8(b_q.data_ptr(), bp, sb, out.data_ptr(), op, so, n, h, w, hb, wb, C,
                                                _lib.current_stream_ptr(b_q.device))
    _lib.check(st, "bevops_upsample_bilinear_s8")
    return out
