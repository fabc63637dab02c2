"""Detection decode on the device (csrc/decode.hip): raw head outputs -> boxes, scores, labels.

`nms_free_decode` is NMSFreeCoder.decode_single (third_party/bev_mmdet3d/core/bbox/coders/nms_free_coder.py:42-98)
for every batch item, optionally with the `z -= h / 2` of BEVFormerHead.get_bboxes (bevformer_head.py:556);
`centerpoint_decode` is CenterHead.get_bboxes up to the NMS (centerpoint_head.py:716-746) with
CenterPointBBoxCoder.decode (centerpoint_bbox_coders.py:138-230).  Neither is one of the reference's 13 registry
functions, so neither is in TRT_FUNCTIONS.

Ranking rule: candidates rank by their fp32 logit, larger first; equal logits rank by lower flat index first
(query * num_classes + class; class * H * W + cell).  include/bevops.h and design/postprocess.md state it in full.

`padded=True` returns the fixed-size tensors the kernels write -- boxes [B, max_num, 9] fp32, scores [B, max_num]
fp32, labels [B, max_num] int32, count [B] int32; kept rows first, in rank order, rows at and behind count[b] zero --
with no host synchronisation, so the call can sit inside a captured graph.  `padded=False` reads `count` (one
synchronisation) and returns one dict {"bboxes", "scores", "labels"} per batch item, trimmed like the reference's.
"""
import ctypes

import torch

from ..utils import lib as _lib
from ..utils import workspace as _ws


def _range6(post_center_range):
    vals = [float(v) for v in (post_center_range.tolist() if torch.is_tensor(post_center_range) else post_center_range)]
    if len(vals) != 6:
        raise ValueError(f"post_center_range needs 6 values, got {len(vals)}")
    return (ctypes.c_float * 6)(*vals)


def _threshold(score_threshold):
    # `if self.score_threshold:` in both coders: None and 0 mean "no score test"
    return float(score_threshold) if score_threshold else -1.0


def _outputs(empty, batch, cap, cols, device, index=False):
    """The fixed-size tensors an entry writes: boxes [batch, cap, cols], scores, labels, count and, on request, index.
    empty: the calling module's torch.empty (every wrapper allocates through its own `torch` name, which the
    buffer-contract tests replace by an arena)."""
    cap = max(cap, 0)
    out = (empty(batch, cap, cols, dtype=torch.float32, device=device), empty(batch, cap, dtype=torch.float32, device=device),
           empty(batch, cap, dtype=torch.int32, device=device), empty(batch, dtype=torch.int32, device=device))
    return out + (empty(batch, cap, dtype=torch.int32, device=device),) if index else out


def _trim(boxes, scores, labels, count, index=None, columns=None):
    """Padded tensors -> one dict per batch item, cut at count[b] (one synchronisation) and to `columns` box columns."""
    out = []
    for b, n in enumerate(count.tolist()):
        d = {"bboxes": boxes[b, :n, :columns], "scores": scores[b, :n], "labels": labels[b, :n]}
        if index is not None:
            d["index"] = index[b, :n]
        out.append(d)
    return out


def nms_free_decode(cls_logits, bbox_preds, max_num, post_center_range, score_threshold=None, bottom_center=False,
                    padded=False):
    """cls_logits [B, num_query, num_classes] (or [num_query, num_classes]), bbox_preds [B, num_query, 10]
    (cx, cy, log w, log l, cz, log h, sin, cos, vx, vy), fp32 or fp16 on the GPU; num_query * num_classes <= 16 384.
    score_threshold: None / 0 = none, else the reference's test with its x0.9 relaxation.  bottom_center: also apply
    get_bboxes' z -= h / 2.  Labels are int32."""
    assert cls_logits.is_cuda and bbox_preds.is_cuda, "nms_free_decode: tensors must be on the GPU"
    if cls_logits.ndim == 2:
        cls_logits, bbox_preds = cls_logits[None], bbox_preds[None]
    if cls_logits.ndim != 3 or bbox_preds.ndim != 3 or bbox_preds.shape[-1] != 10 or \
            bbox_preds.shape[:2] != cls_logits.shape[:2]:
        raise ValueError(f"nms_free_decode: shapes {tuple(cls_logits.shape)}, {tuple(bbox_preds.shape)} do not match "
                         "[B, num_query, num_classes], [B, num_query, 10]")
    if bbox_preds.dtype != cls_logits.dtype or bbox_preds.device != cls_logits.device:
        raise TypeError("nms_free_decode: cls_logits and bbox_preds differ in dtype or device")
    B, nq, nc = cls_logits.shape
    dt = _lib.torch_dtype_code(cls_logits)
    max_num = int(max_num)
    rng = _range6(post_center_range)
    cls, box = cls_logits.contiguous(), bbox_preds.contiguous()
    boxes, scores, labels, count = _outputs(torch.empty, B, max_num, 9, cls.device)
    handle = _lib.load_library()
    with torch.cuda.device(cls.device):
        st = handle.bevops_nms_free_decode(dt, cls.data_ptr(), box.data_ptr(), boxes.data_ptr(), scores.data_ptr(),
                                           labels.data_ptr(), count.data_ptr(), B, nq, nc, max_num, rng,
                                           _threshold(score_threshold), int(bool(bottom_center)),
                                           _lib.current_stream_ptr(cls.device))
    _lib.check(st, "bevops_nms_free_decode")
    return (boxes, scores, labels, count) if padded else _trim(boxes, scores, labels, count)


def _map_strides(t, name):
    """(tensor, channel stride, pixel stride) of a [B, C, H, W] map the kernel can read in place: contiguous NCHW or
    channels-last, every batch item dense; for B == 1 also a channel slice of a wider channels-last tensor (strides
    (., 1, W * Ct, Ct) with Ct >= C: BEVDet's packed head output), passed with channel stride 1 and pixel stride Ct --
    the kernel reads the maps element by element and assumes no alignment of a map's base pointer, and with one batch
    item its batch offset is never applied.  Anything else is made contiguous first."""
    B, C, H, W = t.shape
    if t.is_contiguous():
        return t, H * W, 1
    if t.is_contiguous(memory_format=torch.channels_last):
        return t, 1, C
    if B == 1 and H * W > 0:
        ct = t.stride(3) if W > 1 else (t.stride(2) if H > 1 else C)
        if ct >= C and (C == 1 or t.stride(1) == 1) and (W == 1 or t.stride(3) == ct) and (H == 1 or t.stride(2) == W * ct):
            return t, 1, ct
    return t.contiguous(), H * W, 1


def _slice_strides(t):
    """(channel, pixel, item) strides of a [B, C, H, W] map with B > 1 that is a channel slice of ONE wider
    channels-last tensor [B, H, W, Ct] (strides (H * W * Ct, 1, W * Ct, Ct), Ct > C) -- a batch of BEVDet's packed head
    output -- for bevops_centerpoint_decode_ex; None for anything else (dense maps keep the plain entry)."""
    B, C, H, W = t.shape
    if B < 2 or H * W == 0 or t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last):
        return None
    ct = t.stride(3) if W > 1 else (t.stride(2) if H > 1 else 0)
    if ct > C and (C == 1 or t.stride(1) == 1) and (W == 1 or t.stride(3) == ct) and (H == 1 or t.stride(2) == W * ct) \
            and t.stride(0) == H * W * ct:
        return 1, ct, H * W * ct
    return None


def centerpoint_decode(reg, height, dim, rot, vel, heatmap, max_num, post_center_range, pc_range, out_size_factor,
                       voxel_size, score_threshold=None, norm_bbox=True, heatmap_is_score=False, padded=False):
    """The six head maps of BEVDet.forward, [B, c, H, W] with c = 2, 1, 3, 2, 2, num_classes, fp32 or fp16 on the GPU,
    contiguous or channels-last (read in place).  vel may be None (7-column boxes; the padded tensor keeps 9 columns,
    the last two zero), reg may be None (cell centre, + 0.5).  pc_range / voxel_size: their first two values are used.
    norm_bbox: dim holds logarithms (CenterHead.norm_bbox).  heatmap_is_score: the map holds scores already (what
    CenterPointBBoxCoder.decode is handed), ranked and reported as they are.  max_num <= 4 096.  Labels are int32."""
    maps = [reg, height, dim, rot, vel, heatmap]
    names = ["reg", "height", "dim", "rot", "vel", "heatmap"]
    chans = [2, 1, 3, 2, 2, heatmap.shape[1] if heatmap is not None and heatmap.ndim == 4 else -1]
    if heatmap is None or height is None or dim is None or rot is None:
        raise ValueError("centerpoint_decode: height, dim, rot and heatmap are required")
    assert heatmap.is_cuda, "centerpoint_decode: tensors must be on the GPU"
    if heatmap.ndim != 4:
        raise ValueError(f"centerpoint_decode: heatmap must be [B, num_classes, H, W], got {tuple(heatmap.shape)}")
    B, nc, H, W = heatmap.shape
    dt = _lib.torch_dtype_code(heatmap)
    ptrs, strides, items = [], [], []
    keep = []
    for t, name, c in zip(maps, names, chans):
        if t is None:
            ptrs.append(None)
            strides.append((1, 1))
            items.append(c * H * W)
            continue
        if tuple(t.shape) != (B, c, H, W):
            raise ValueError(f"centerpoint_decode: {name} must be {(B, c, H, W)}, got {tuple(t.shape)}")
        if t.dtype != heatmap.dtype or t.device != heatmap.device:
            raise TypeError(f"centerpoint_decode: {name} differs from heatmap in dtype or device")
        sliced = _slice_strides(t)
        if sliced is not None:
            cs, ps, item = sliced
        else:
            t, cs, ps = _map_strides(t, name)
            item = None
        keep.append(t)
        ptrs.append(t.data_ptr())
        strides.append((cs, ps))
        items.append(item)
    # B > 1 channel slices of a wider channels-last tensor carry their own batch-item stride: the _ex entry
    ex = any(s is not None for s, t in zip(items, maps) if t is not None)
    max_num = int(max_num)
    rng = _range6(post_center_range)
    if ex:
        flat = [v for (cs, ps), item, c in zip(strides, items, chans) for v in (cs, ps, c * H * W if item is None else item)]
        strides_c = (ctypes.c_int64 * 18)(*flat)
    else:
        strides_c = (ctypes.c_int32 * 12)(*(v for pair in strides for v in pair))
    boxes, scores, labels, count = _outputs(torch.empty, B, max_num, 9, heatmap.device)
    handle = _lib.load_library()
    stream = _lib.current_stream_ptr(heatmap.device)
    nws = handle.bevops_centerpoint_decode_workspace_size(B, nc, H, W, max_num)
    ws = _ws.lend("centerpoint_decode", nws, heatmap.device, stream) if nws else None
    entry = handle.bevops_centerpoint_decode_ex if ex else handle.bevops_centerpoint_decode
    with torch.cuda.device(heatmap.device):
        st = entry(
            dt, *ptrs, strides_c, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), count.data_ptr(), B, nc, H, W,
            max_num, float(out_size_factor), float(voxel_size[0]), float(voxel_size[1]), float(pc_range[0]),
            float(pc_range[1]), rng, _threshold(score_threshold), int(bool(norm_bbox)), int(bool(heatmap_is_score)),
            ws.data_ptr() if ws is not None else None, nws, stream)
    _lib.check(st, "bevops_centerpoint_decode")
    if padded:
        return boxes, scores, labels, count
    return _trim(boxes, scores, labels, count, columns=9 if vel is not None else 7)
