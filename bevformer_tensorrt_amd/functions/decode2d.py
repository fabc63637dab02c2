"""2-D detection decode on the device: CenterNet and YOLOX (csrc/decode2d.hip) and the axis-aligned batched NMS (the box
entry of csrc/nms.hip).

`centernet_decode` is mmdet 2.x's CenterNetHead.get_bboxes (decode_heatmap: local maximum, top k, box, border, rescale),
`yolox_decode` is YOLOXHead.get_bboxes up to the NMS (_bbox_decode, score, label), `box_nms` is mmcv's batched_nms with
mmdet's valid_mask in front -- as the reference's detectors call them (det2trt/models/detector/{centernet,yolox}.py:
post_process).  The statement is written from the published algorithm; parity with the libraries themselves is
unpinned (include/bevops.h, design/postprocess.md).  None of the three is one of the reference's 13 registry functions,
so none is in TRT_FUNCTIONS.

Ranking rule, as for the 3-D decoders: larger value first, equal values by lower flat index (CenterNet:
class * H * W + y * W + x; NMS: input row) first.

`padded=True` returns the fixed-size tensors the kernels write, with no host synchronisation, so the call can sit inside
a captured graph; `padded=False` reads `count` (one synchronisation) and returns one dict per batch item.  CPU tensors
go to the torch statements in postprocess.py.
"""
import ctypes

import torch

from ..utils import lib as _lib
from ..utils import workspace as _ws
from .decode import _map_strides, _outputs, _trim
from .nms import _nms_inputs


def _rows(values, batch, width, name):
    """None, or host floats as an fp32 CPU tensor [batch, width] (a single row is repeated for every item)."""
    if values is None:
        return None
    t = torch.as_tensor(values, dtype=torch.float32).detach().cpu()
    if t.numel() == width:
        t = t.reshape(1, width).expand(batch, width)
    if tuple(t.shape) != (batch, width):
        raise ValueError(f"{name} must be [{batch}, {width}]")
    return t


def _c_rows(rows):
    if rows is None:
        return None
    flat = rows.flatten().tolist()
    return (ctypes.c_float * len(flat))(*flat)


def centernet_decode(heatmap, wh, offset, k, input_shape, kernel=3, border=None, scale_factor=None, score_threshold=None,
                     padded=False):
    """heatmap [B, C, H, W] SCORES (after the head's sigmoid), wh [B, 2, H, W], offset [B, 2, H, W]; fp32 or fp16,
    contiguous or channels-last (read in place).  input_shape = (inp_h, inp_w), mmdet's batch_input_shape.  border: None
    or per image (border_x, border_y) = mmdet's border[2], border[0]; scale_factor: None (no rescale) or per image
    four factors.  score_threshold: None = none (mmdet), else rows with score > threshold are kept.  kernel 1, 3, 5, 7;
    k <= min(4 096, C H W); C H W <= 2^24; B <= 64.  Boxes [B, k, 4] (tl_x, tl_y, br_x, br_y); labels int32."""
    if heatmap.ndim != 4:
        raise ValueError(f"centernet_decode: heatmap must be [B, C, H, W], got {tuple(heatmap.shape)}")
    B, C, H, W = heatmap.shape
    for t, name in ((wh, "wh"), (offset, "offset")):
        if tuple(t.shape) != (B, 2, H, W):
            raise ValueError(f"centernet_decode: {name} must be {(B, 2, H, W)}, got {tuple(t.shape)}")
        if t.dtype != heatmap.dtype or t.device != heatmap.device:
            raise TypeError(f"centernet_decode: {name} differs from heatmap in dtype or device")
    border, scale = _rows(border, B, 2, "border"), _rows(scale_factor, B, 4, "scale_factor")
    inp_h, inp_w = int(input_shape[0]), int(input_shape[1])
    k = int(k)
    if not heatmap.is_cuda:
        from ..postprocess import centernet_decode_torch
        out = centernet_decode_torch(heatmap, wh, offset, k, (inp_h, inp_w), kernel, border, scale, score_threshold)
        return out if padded else _trim(*out)
    dt = _lib.torch_dtype_code(heatmap)
    ptrs, strides, keep = [], [], []
    for t, name in ((heatmap, "heatmap"), (wh, "wh"), (offset, "offset")):
        t, cs, ps = _map_strides(t, name)
        keep.append(t)
        ptrs.append(t.data_ptr())
        strides += [cs, ps]
    dev = heatmap.device
    boxes, scores, labels, count = _outputs(torch.empty, B, k, 4, dev)
    handle = _lib.load_library()
    stream = _lib.current_stream_ptr(dev)
    nws = handle.bevops_centernet_decode_workspace_size(B, C, H, W, k)
    ws = _ws.lend("centernet_decode", max(nws, 8), dev, stream)
    thr = -1.0 if score_threshold is None else float(score_threshold)
    with torch.cuda.device(dev):
        st = handle.bevops_centernet_decode(dt, *ptrs, (ctypes.c_int32 * 6)(*strides), boxes.data_ptr(), scores.data_ptr(),
                                            labels.data_ptr(), count.data_ptr(), B, C, H, W, k, int(kernel), inp_h, inp_w,
                                            _c_rows(border), _c_rows(scale), thr, ws.data_ptr(), nws, stream)
    _lib.check(st, "bevops_centernet_decode")
    return (boxes, scores, labels, count) if padded else _trim(boxes, scores, labels, count)


def yolox_decode(cls_scores, bbox_preds, objectnesses, strides=(8, 16, 32), scale_factor=None):
    """Per level l: cls_scores[l] [B, C, H_l, W_l], bbox_preds[l] [B, 4, H_l, W_l], objectnesses[l] [B, 1, H_l, W_l],
    all logits, fp32 or fp16, contiguous or channels-last; strides[l] the level's integer stride.  scale_factor: None
    or per image four factors (the boxes are divided by them, before any NMS).  Returns boxes [B, P, 4], scores
    [B, P], labels [B, P] int32 in prior order (level-major, row, column): fixed shapes, no synchronisation."""
    L = len(cls_scores)
    if not (L == len(bbox_preds) == len(objectnesses) == len(strides)) or L < 1:
        raise ValueError("yolox_decode: cls_scores, bbox_preds, objectnesses and strides must have one entry per level")
    first = cls_scores[0]
    B, C = first.shape[0], first.shape[1]
    for l in range(L):
        H, W = cls_scores[l].shape[-2:]
        for t, c, name in ((cls_scores[l], C, "cls_scores"), (bbox_preds[l], 4, "bbox_preds"),
                           (objectnesses[l], 1, "objectnesses")):
            if tuple(t.shape) != (B, c, H, W):
                raise ValueError(f"yolox_decode: {name}[{l}] must be {(B, c, H, W)}, got {tuple(t.shape)}")
            if t.dtype != first.dtype or t.device != first.device:
                raise TypeError(f"yolox_decode: {name}[{l}] differs from cls_scores[0] in dtype or device")
    scale = _rows(scale_factor, B, 4, "scale_factor")
    strides = [int(s) for s in strides]
    if not first.is_cuda:
        from ..postprocess import yolox_decode_torch
        return yolox_decode_torch(cls_scores, bbox_preds, objectnesses, strides, scale)
    dt = _lib.torch_dtype_code(first)
    ptrs, shapes, pairs, keep = [[], [], []], [], [], []
    for l in range(L):
        H, W = cls_scores[l].shape[-2:]
        shapes += [H, W, strides[l]]
        for which, t in enumerate((cls_scores[l], bbox_preds[l], objectnesses[l])):
            t, cs, ps = _map_strides(t, "map")
            keep.append(t)
            ptrs[which].append(t.data_ptr())
            pairs += [cs, ps]
    P = sum(shapes[0::3][l] * shapes[1::3][l] for l in range(L))
    dev = first.device
    boxes = torch.empty(B, P, 4, dtype=torch.float32, device=dev)
    scores = torch.empty(B, P, dtype=torch.float32, device=dev)
    labels = torch.empty(B, P, dtype=torch.int32, device=dev)
    handle = _lib.load_library()
    arr = lambda p: (ctypes.c_void_p * L)(*p)
    with torch.cuda.device(dev):
        st = handle.bevops_yolox_decode(dt, arr(ptrs[0]), arr(ptrs[1]), arr(ptrs[2]), (ctypes.c_int32 * (3 * L))(*shapes),
                                        (ctypes.c_int32 * (6 * L))(*pairs), boxes.data_ptr(), scores.data_ptr(),
                                        labels.data_ptr(), B, L, C, _c_rows(scale), _lib.current_stream_ptr(dev))
    _lib.check(st, "bevops_yolox_decode")
    return boxes, scores, labels


def box_nms(boxes, scores, labels, count=None, *, score_threshold=None, iou_threshold, class_aware=True, max_out=None,
            padded=False):
    """boxes [B, N, 4] fp32 (x1, y1, x2, y2), scores [B, N] fp32, labels [B, N] int32, count [B] int32 or None (= N)
    (one item may come without the batch axis).  Candidates: rows below count with score >= score_threshold (None =
    every row).  Row j is suppressed by an earlier kept row i when IoU > iou_threshold and, with class_aware, the
    labels are equal.  N <= 16 384, 1 <= max_out <= N (None = N).  Returns boxes [B, max_out, 4], scores, labels,
    count [B], index [B, max_out] int32 (input rows), kept rows first in rank order, zero behind count."""
    boxes, scores, labels, count = _nms_inputs("box_nms", 4, boxes, scores, labels, count)
    B, N = scores.shape
    post = N if max_out is None else int(max_out)
    thr = float("-inf") if score_threshold is None else float(score_threshold)
    if not boxes.is_cuda:
        from ..postprocess import box_nms_torch
        out = box_nms_torch(boxes, scores, labels, count, score_threshold=thr, iou_threshold=iou_threshold,
                            class_aware=class_aware, max_out=post)
        return out if padded else _trim(*out)
    dev = boxes.device
    out_b, out_s, out_l, out_c, out_i = _outputs(torch.empty, B, post, 4, dev, index=True)
    handle = _lib.load_library()
    stream = _lib.current_stream_ptr(dev)
    nws = handle.bevops_box_nms_workspace_size(B, N)
    ws = _ws.lend("box_nms", max(nws, 8), dev, stream)
    with torch.cuda.device(dev):
        st = handle.bevops_box_nms(boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                                   count.data_ptr() if count is not None else None, out_b.data_ptr(), out_s.data_ptr(),
                                   out_l.data_ptr(), out_c.data_ptr(), out_i.data_ptr(), B, N, thr, float(iou_threshold),
                                   int(bool(class_aware)), post, ws.data_ptr(), nws, stream)
    _lib.check(st, "bevops_box_nms")
    return (out_b, out_s, out_l, out_c, out_i) if padded else _trim(out_b, out_s, out_l, out_c, out_i)
