"""BEV non-maximum suppression on the device (the BEV entry of csrc/nms.hip): what CenterHead.get_bboxes does behind the
coder.

`bev_nms` is the batched face of `bevops_bev_nms`: the rotated scale-NMS of CenterHead.get_task_detections
(third_party/bev_mmdet3d/models/dense_heads/centerpoint_head.py:808-905) or the circle NMS of get_bboxes (:750-773),
the size restore and, on request, the z shift of :793.  `nms_bev` and `circle_nms` carry the signatures of
third_party/bev_mmdet3d/core/post_processing/box3d_nms.py:227-273 and :182-221; `bev_iou` exposes the pair test.
None of them is one of the reference's 13 registry functions, so none is in TRT_FUNCTIONS.

Ranking: descending score, equal scores by lower input row first (include/bevops.h, design/postprocess.md).
CPU tensors go to the torch statement in postprocess.py (`bev_nms_torch`), which evaluates the pair test in fp64.

`padded=True` returns what the kernels write -- boxes [B, post_max_size, 9] fp32, scores, labels int32
[B, post_max_size], count [B] int32, index [B, post_max_size] int32 (kept rows as row numbers of the input); kept rows
first, in rank order, zero behind count[b] -- with no host synchronisation, so the call can sit in a captured graph
behind `centerpoint_decode(..., padded=True)`.  `padded=False` reads `count` (one synchronisation) and returns one
dict {"bboxes", "scores", "labels", "index"} per batch item.
"""
import ctypes

import numpy as np
import torch

from ..utils import lib as _lib
from ..utils import workspace as _ws
from .decode import _outputs, _trim

_MODES = {"rotate": 0, "circle": 1}


def _factors(rescale_factor):
    """None / scalar / per-label list -> list of floats (empty = no scaling)."""
    if rescale_factor is None:
        return []
    if torch.is_tensor(rescale_factor) or isinstance(rescale_factor, np.ndarray):
        rescale_factor = rescale_factor.tolist()
    if isinstance(rescale_factor, (list, tuple)):
        return [float(v) for v in rescale_factor]
    return [float(rescale_factor)]


def _nms_inputs(name, width, boxes, scores, labels, count):
    """What `bev_nms` and `box_nms` do with their inputs: lift a single item to a batch of one, check the shapes
    [B, N, width], [B, N], [B, N] and, for device tensors, dtypes, count and devices, and make them contiguous."""
    if boxes.ndim == 2:
        boxes, scores, labels = boxes[None], scores[None], labels[None]
        count = None if count is None else count.reshape(1)
    if boxes.ndim != 3 or boxes.shape[-1] != width or scores.shape != boxes.shape[:2] or labels.shape != boxes.shape[:2]:
        raise ValueError(f"{name}: shapes {tuple(boxes.shape)}, {tuple(scores.shape)}, {tuple(labels.shape)} do not "
                         f"match [B, N, {width}], [B, N], [B, N]")
    if not boxes.is_cuda:   # the torch statement takes them as they are
        return boxes, scores, labels, count
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32 or labels.dtype != torch.int32:
        raise TypeError(f"{name}: boxes and scores must be float32, labels int32")
    if count is not None and (count.dtype != torch.int32 or count.shape != boxes.shape[:1]):
        raise TypeError(f"{name}: count must be int32 [B]")
    for t in (scores, labels, count):
        if t is not None and t.device != boxes.device:
            raise TypeError(f"{name}: tensors on different devices")
    return boxes.contiguous(), scores.contiguous(), labels.contiguous(), None if count is None else count.contiguous()


def bev_nms(boxes, scores, labels, count=None, *, nms_type="rotate", threshold, pre_max_size=None, post_max_size,
            rescale_factor=None, bottom_center=False, padded=False):
    """boxes [B, N, 9] fp32 (x, y, z, w, l, h, yaw, vx, vy), scores [B, N] fp32, labels [B, N] int32, count [B] int32
    or None (= N): the padded 4-tuple of `centerpoint_decode` as it is (one item may come without the batch axis).
    nms_type "rotate": threshold is the IoU above which a row is suppressed; "circle": the value the SQUARED centre
    distance is compared with (circle_nms does not square min_radius, so neither does this).  rescale_factor: None, a
    scalar or one factor per label (nms_rescale_factor); sizes come back as fl(fl(d f) / f), as the reference's
    multiply and divide leave them.  bottom_center: z -= h / 2 (get_bboxes).  N <= 4 096, 1 <= post_max_size <= N."""
    if nms_type not in _MODES:
        raise ValueError(f"bev_nms: nms_type must be 'rotate' or 'circle', got {nms_type!r}")
    boxes, scores, labels, count = _nms_inputs("bev_nms", 9, boxes, scores, labels, count)
    if not boxes.is_cuda:
        from ..postprocess import bev_nms_torch
        out = bev_nms_torch(boxes, scores, labels, count, nms_type=nms_type, threshold=threshold,
                            pre_max_size=pre_max_size, post_max_size=post_max_size, rescale_factor=rescale_factor,
                            bottom_center=bottom_center)
        return out if padded else _trim(*out)
    B, N = scores.shape
    post = int(post_max_size)
    fac = _factors(rescale_factor)
    fac_c = (ctypes.c_float * max(len(fac), 1))(*fac)
    dev = boxes.device
    out_b, out_s, out_l, out_c, out_i = _outputs(torch.empty, B, post, 9, dev, index=True)
    handle = _lib.load_library()
    stream = _lib.current_stream_ptr(dev)
    nws = handle.bevops_bev_nms_workspace_size(B, N)
    ws = _ws.lend("bev_nms", max(nws, 8), dev, stream)
    with torch.cuda.device(dev):
        st = handle.bevops_bev_nms(_MODES[nms_type], boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                                   count.data_ptr() if count is not None else None, out_b.data_ptr(), out_s.data_ptr(),
                                   out_l.data_ptr(), out_c.data_ptr(), out_i.data_ptr(), B, N,
                                   int(pre_max_size) if pre_max_size is not None else 0, post, float(threshold),
                                   fac_c, len(fac), int(bool(bottom_center)), ws.data_ptr(), nws, stream)
    _lib.check(st, "bevops_bev_nms")
    return (out_b, out_s, out_l, out_c, out_i) if padded else _trim(out_b, out_s, out_l, out_c, out_i)


def _xywhr(boxes, xyxyr2xywhr):
    if not xyxyr2xywhr:
        return boxes
    return torch.stack(((boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2, boxes[:, 2] - boxes[:, 0],
                        boxes[:, 3] - boxes[:, 1], boxes[:, 4]), dim=-1)          # box3d_nms.py:257-267


def nms_bev(boxes, scores, thresh, pre_max_size=None, post_max_size=None, xyxyr2xywhr=True):
    """box3d_nms.py:227-273: boxes [N, 5] (x1, y1, x2, y2, ry), or (x, y, w, l, ry) with xyxyr2xywhr=False; scores [N].
    Returns the kept rows as int64 indices into the input, in rank order.  The length depends on the data, so this
    wrapper synchronises once (it reads the count); `bev_nms(..., padded=True)` is the form without."""
    assert boxes.size(1) == 5, "Input boxes shape should be [N, 5]"
    n = boxes.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=boxes.device)
    xywhr = _xywhr(boxes.float(), xyxyr2xywhr)
    full = torch.zeros(n, 9, dtype=torch.float32, device=boxes.device)
    full[:, [0, 1, 3, 4, 6]] = xywhr
    pre = None if pre_max_size is None else max(int(pre_max_size), 0)
    if pre == 0:
        return torch.zeros(0, dtype=torch.int64, device=boxes.device)
    post = n if post_max_size is None else min(int(post_max_size), n)
    if post <= 0:
        return torch.zeros(0, dtype=torch.int64, device=boxes.device)
    out = bev_nms(full, scores.float().reshape(-1), torch.zeros(n, dtype=torch.int32, device=boxes.device),
                  nms_type="rotate", threshold=thresh, pre_max_size=pre, post_max_size=post, padded=True)
    return out[4][0, :int(out[3][0])].to(torch.int64)


def circle_nms(dets, thresh, post_max_size=83):
    """box3d_nms.py:182-221: dets [N, 3] (x, y, score), tensor or numpy; thresh is compared with the SQUARED distance.
    Returns the kept rows in rank order: a tensor for a tensor, a list of ints for numpy (as the reference's; numpy
    input is host data and takes the CPU statement).  Synchronises once."""
    is_np = isinstance(dets, np.ndarray)
    d = torch.from_numpy(np.ascontiguousarray(dets, np.float32)) if is_np else dets.float()
    n = d.shape[0]
    post = min(int(post_max_size), n)
    if n == 0 or post <= 0:
        return [] if is_np else torch.zeros(0, dtype=torch.int64, device=d.device)
    full = torch.zeros(n, 9, dtype=torch.float32, device=d.device)
    full[:, :2] = d[:, :2]
    out = bev_nms(full, d[:, 2].contiguous(), torch.zeros(n, dtype=torch.int32, device=d.device), nms_type="circle",
                  threshold=thresh, post_max_size=post, padded=True)
    keep = out[4][0, :int(out[3][0])].to(torch.int64)
    return keep.cpu().tolist() if is_np else keep


def bev_iou(boxes_a, boxes_b):
    """boxes_a [M, 5], boxes_b [N, 5] as (x, y, w, l, yaw) -> IoU [M, N] fp32: the pair test of the rotate mode
    (exact overlap of the two rotated rectangles, evaluated relative to the a-box's centre)."""
    if boxes_a.ndim != 2 or boxes_b.ndim != 2 or boxes_a.shape[1] != 5 or boxes_b.shape[1] != 5:
        raise ValueError(f"bev_iou: shapes {tuple(boxes_a.shape)}, {tuple(boxes_b.shape)} do not match [M, 5], [N, 5]")
    if not boxes_a.is_cuda:
        from ..postprocess import bev_iou_fp64
        return bev_iou_fp64(boxes_a, boxes_b).float()
    a, b = boxes_a.float().contiguous(), boxes_b.to(boxes_a.device).float().contiguous()
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
    if out.numel() == 0:
        return out
    handle = _lib.load_library()
    with torch.cuda.device(a.device):
        st = handle.bevops_bev_iou(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], out.data_ptr(),
                                   _lib.current_stream_ptr(a.device))
    _lib.check(st, "bevops_bev_iou")
    return out
