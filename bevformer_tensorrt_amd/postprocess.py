"""Box coders of the two detectors: head outputs -> boxes, scores, labels.

`NMSFreeCoder` and `CenterPointBBoxCoder` take the constructor arguments of the reference's classes
(third_party/bev_mmdet3d/core/bbox/coders/nms_free_coder.py:23-36, centerpoint_bbox_coders.py:25-43) and offer the
same `decode(...)`.  Device tensors go to the HIP kernels (functions/decode.py, csrc/decode.hip); CPU tensors go to
the torch restatement below, written from the algorithm: it is the CPU statement of what the kernels compute and what
the tests compare them with.

Ranking rule, both paths: candidates rank by their fp32 logit (or, where a coder is handed scores, by that value),
larger first; equal values rank by lower flat index first (NMS-free: query * num_classes + class; CenterPoint:
class * H * W + row * W + col).  torch.topk leaves the order among equals unspecified, so the restatement uses a
stable descending sort.

Both paths produce the padded form first -- boxes [B, max_num, 9] fp32, scores [B, max_num] fp32, labels
[B, max_num] int32, count [B] int32, kept rows in rank order at the front, zero behind -- and the per-item dicts of the
reference are cut from it.  BEVDet's rotated scale-NMS and the circle NMS (CenterHead.get_task_detections, get_bboxes)
follow the CenterPoint coder: `bev_nms_torch` below is their CPU statement, with the pair test in fp64 -- the
definition ("the exact overlapping area of the two boxes", box3d_nms.py:230-231) that the kernel's fp32 evaluation is
measured against.
"""
import torch

from .functions.decode import nms_free_decode, centerpoint_decode
from .functions.decode2d import _rows
from .functions.nms import _factors


def _rank(values, max_num):
    """Flat indices [B, max_num] of the top max_num of values [B, n] under the ranking rule."""
    values = values.float() + 0.0          # -0 ranks as +0
    return torch.sort(values, dim=1, descending=True, stable=True).indices[:, :max_num]


def _pad(keep, boxes, scores, labels):
    """Compaction of the kept rows to the front, zeros behind: [B, K, .] -> the padded form."""
    B, K = keep.shape
    out_b, out_s = torch.zeros(B, K, 9), torch.zeros(B, K)
    out_l, count = torch.zeros(B, K, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        n = int(keep[b].sum())
        out_b[b, :n, :boxes.shape[-1]] = boxes[b][keep[b]]
        out_s[b, :n] = scores[b][keep[b]]
        out_l[b, :n] = labels[b][keep[b]].to(torch.int32)
        count[b] = n
    return out_b, out_s, out_l, count


def _in_range(centres, post_center_range):
    r = torch.tensor([float(v) for v in post_center_range], dtype=torch.float32)
    return (centres >= r[:3]).all(-1) & (centres <= r[3:]).all(-1)


def nms_free_decode_torch(cls_logits, bbox_preds, max_num, post_center_range, score_threshold=None,
                          bottom_center=False, return_index=False):
    """The padded result of `nms_free_decode` in torch ops on the CPU.  return_index: also the selected flat indices
    [B, max_num] in rank order (before the masks) and the keep mask [B, max_num]."""
    cls, box = cls_logits.detach().float().cpu(), bbox_preds.detach().float().cpu()
    if cls.ndim == 2:
        cls, box = cls[None], box[None]
    B, nq, nc = cls.shape
    if not 1 <= max_num <= nq * nc:
        raise ValueError(f"max_num {max_num} outside 1 .. {nq * nc}")
    index = _rank(cls.reshape(B, -1), max_num)
    scores = torch.gather(cls.reshape(B, -1), 1, index).sigmoid()
    labels = index % nc
    query = torch.div(index, nc, rounding_mode="trunc")
    p = torch.gather(box, 1, query[..., None].expand(B, max_num, 10))
    boxes = torch.cat([p[..., 0:2], p[..., 4:5], p[..., 2:4].exp(), p[..., 5:6].exp(),
                       torch.atan2(p[..., 6:7], p[..., 7:8]), p[..., 8:10]], dim=-1)
    keep = _in_range(boxes[..., :3], post_center_range)
    if score_threshold:
        for b in range(B):       # nms_free_coder.py:67-75, per item
            mask = scores[b] > score_threshold
            tmp = score_threshold
            while mask.sum() == 0:
                tmp *= 0.9
                if tmp < 0.01:
                    mask = scores[b] > -1
                    break
                mask = scores[b] >= tmp
            keep[b] &= mask
    if bottom_center:
        boxes[..., 2] = boxes[..., 2] - boxes[..., 5] * 0.5
    out = _pad(keep, boxes, scores, labels)
    return out + (index, keep) if return_index else out


def centerpoint_decode_torch(reg, height, dim, rot, vel, heatmap, max_num, post_center_range, pc_range, out_size_factor,
                             voxel_size, score_threshold=None, norm_bbox=True, heatmap_is_score=False,
                             return_index=False):
    """The padded result of `centerpoint_decode` in torch ops on the CPU."""
    f = lambda t: None if t is None else t.detach().float().cpu()
    reg, height, dim, rot, vel, heat = (f(t) for t in (reg, height, dim, rot, vel, heatmap))
    B, nc, H, W = heat.shape
    if not 1 <= max_num <= nc * H * W:
        raise ValueError(f"max_num {max_num} outside 1 .. {nc * H * W}")
    flat = heat.reshape(B, -1)
    index = _rank(flat, max_num)
    scores = torch.gather(flat, 1, index)
    if not heatmap_is_score:
        scores = scores.sigmoid()
    labels = torch.div(index, H * W, rounding_mode="trunc")
    cell = index % (H * W)
    ys, xs = torch.div(cell, W, rounding_mode="trunc").float(), (cell % W).float()

    def at(t):      # [B, c, H, W] -> [B, max_num, c] at the winning cells
        c = t.shape[1]
        return torch.gather(t.reshape(B, c, H * W), 2, cell[:, None, :].expand(B, c, max_num)).transpose(1, 2)

    if reg is not None:
        r = at(reg)
        xs, ys = xs + r[..., 0], ys + r[..., 1]
    else:
        xs, ys = xs + 0.5, ys + 0.5
    xs = xs * out_size_factor * voxel_size[0] + pc_range[0]
    ys = ys * out_size_factor * voxel_size[1] + pc_range[1]
    d = at(dim)
    if norm_bbox:
        d = d.exp()
    rt = at(rot)
    cols = [xs[..., None], ys[..., None], at(height), d, torch.atan2(rt[..., 0:1], rt[..., 1:2])]
    if vel is not None:
        cols.append(at(vel))
    boxes = torch.cat(cols, dim=-1)
    keep = _in_range(boxes[..., :3], post_center_range)
    if score_threshold:
        keep &= scores > score_threshold
    out = _pad(keep, boxes, scores, labels)
    return out + (index, keep) if return_index else out


def _clip_half_plane(verts, n, axis, sign, bound):
    """One Sutherland-Hodgman stage for P polygons at once: verts [P, 8, 2], n [P] vertex counts, kept part
    sign * v[axis] <= bound [P].  Returns (verts, n) of the clipped polygons."""
    P = verts.shape[0]
    rows = torch.arange(P)
    out = torch.zeros_like(verts)
    m = torch.zeros(P, dtype=torch.long)
    for k in range(8):
        live = k < n
        cur = verts[:, k]
        nxt = verts[rows, torch.where(k + 1 < n, k + 1, 0)]
        dc, dn = bound - sign * cur[:, axis], bound - sign * nxt[:, axis]
        ic, inx = dc >= 0, dn >= 0
        put = live & ic & (m < 8)
        out[rows[put], m[put]] = cur[put]
        m = m + put.long()
        put = live & (ic != inx) & (m < 8)
        t = torch.where(put, dc / torch.where(put, dc - dn, torch.ones_like(dc)), torch.zeros_like(dc))
        p = cur + t[:, None] * (nxt - cur)
        p[:, axis] = sign * bound
        out[rows[put], m[put]] = p[put]
        m = m + put.long()
    return out, m


def bev_iou_fp64(boxes_a, boxes_b):
    """IoU [M, N] in fp64 of rotated rectangles (x, y, w, l, yaw), w along (cos yaw, sin yaw): rectangle b clipped
    against the four edges of rectangle a in a's frame, area by the shoelace formula.  A pair whose union is not
    positive has IoU 0; NaN inputs give NaN."""
    a, b = boxes_a.detach().double().cpu(), boxes_b.detach().double().cpu()
    M, N = a.shape[0], b.shape[0]
    A, B = a[:, None, :].expand(M, N, 5).reshape(-1, 5), b[None, :, :].expand(M, N, 5).reshape(-1, 5)
    iou = torch.zeros(M * N, dtype=torch.float64)
    d = B[:, :2] - A[:, :2]
    reach = 0.5 * (torch.hypot(A[:, 2], A[:, 3]) + torch.hypot(B[:, 2], B[:, 3]))
    bad = torch.isnan(A).any(1) | torch.isnan(B).any(1)
    near = (d.square().sum(1) <= reach.square() * (1 + 1e-9)) & ~bad
    if near.any():
        A, B, d = A[near], B[near], d[near]
        ca, sa = torch.cos(A[:, 4]), torch.sin(A[:, 4])
        rot = lambda v: torch.stack([v[:, 0] * ca + v[:, 1] * sa, v[:, 1] * ca - v[:, 0] * sa], 1)
        cb, sb = torch.cos(B[:, 4]), torch.sin(B[:, 4])
        e = rot(d)
        u = rot(torch.stack([0.5 * B[:, 2] * cb, 0.5 * B[:, 2] * sb], 1))
        v = rot(torch.stack([-0.5 * B[:, 3] * sb, 0.5 * B[:, 3] * cb], 1))
        verts = torch.zeros(A.shape[0], 8, 2, dtype=torch.float64)
        verts[:, 0], verts[:, 1], verts[:, 2], verts[:, 3] = e + u + v, e - u + v, e - u - v, e + u - v
        n = torch.full((A.shape[0],), 4, dtype=torch.long)
        hw, hl = 0.5 * A[:, 2], 0.5 * A[:, 3]
        for axis, sign, bound in ((0, 1.0, hw), (0, -1.0, hw), (1, 1.0, hl), (1, -1.0, hl)):
            verts, n = _clip_half_plane(verts, n, axis, sign, bound)
        nxt = torch.roll(verts, -1, 1).clone()
        rows = torch.arange(A.shape[0])
        last = (n - 1).clamp(min=0)
        nxt[rows, last] = verts[:, 0]
        cross = verts[..., 0] * nxt[..., 1] - nxt[..., 0] * verts[..., 1]
        cross = torch.where(torch.arange(8)[None, :] < n[:, None], cross, torch.zeros_like(cross))
        inter = torch.where(n >= 3, 0.5 * cross.sum(1).abs(), torch.zeros_like(hw))
        union = A[:, 2] * A[:, 3] + B[:, 2] * B[:, 3] - inter
        iou[near] = torch.where(union > 0, inter / torch.where(union > 0, union, torch.ones_like(union)),
                                torch.zeros_like(union))
    iou[bad] = float("nan")
    return iou.reshape(M, N)


def _greedy_keep(order, suppressed_by, post):
    """The greedy scan both NMS statements share: walk the ranked rows; a row not yet suppressed is kept and suppresses
    what suppressed_by(i) -- a bool vector over the ranks behind i, computed when row i is kept and not before -- marks.
    Stops at `post` kept rows.  Returns the kept rows as entries of `order`."""
    M = order.numel()
    removed = torch.zeros(M, dtype=torch.bool)
    keep = []
    for i in range(M):
        if removed[i]:
            continue
        keep.append(i)
        if len(keep) == post or i + 1 == M:
            break
        removed[i + 1:] |= suppressed_by(i)
    return order[torch.tensor(keep, dtype=torch.long)]


def bev_nms_torch(boxes, scores, labels, count=None, *, nms_type="rotate", threshold, pre_max_size=None,
                  post_max_size, rescale_factor=None, bottom_center=False):
    """The padded result of `bev_nms` -- (boxes [B, post_max_size, 9], scores, labels int32, count, index int32) --
    stated in torch ops on the CPU: stable descending sort (equal scores: lower row first), the sizes multiplied and
    divided back in fp32 as the reference's tensor ops do (centerpoint_head.py:836-876), the pair test in fp64
    (`bev_iou_fp64`; circle: the fp32 expression of box3d_nms.py:216), greedy scan, cut to post_max_size."""
    boxes, scores = boxes.detach().float().cpu(), scores.detach().float().cpu()
    labels = labels.detach().cpu()
    if boxes.ndim == 2:
        boxes, scores, labels = boxes[None], scores[None], labels[None]
        count = None if count is None else count.reshape(1)
    B, N = scores.shape
    post = int(post_max_size)
    if not 1 <= post <= N:
        raise ValueError(f"post_max_size {post} outside 1 .. {N}")
    if nms_type not in ("rotate", "circle"):
        raise ValueError(f"nms_type must be 'rotate' or 'circle', got {nms_type!r}")
    fac = _factors(rescale_factor)
    counts = [N] * B if count is None else [min(max(int(c), 0), N) for c in count.tolist()]
    pre = N if pre_max_size is None or int(pre_max_size) <= 0 else min(int(pre_max_size), N)
    out_b, out_s = torch.zeros(B, post, 9), torch.zeros(B, post)
    out_l, out_i = torch.zeros(B, post, dtype=torch.int32), torch.zeros(B, post, dtype=torch.int32)
    out_c = torch.zeros(B, dtype=torch.int32)
    thr32 = torch.tensor(float(threshold), dtype=torch.float32)
    for b in range(B):
        n = counts[b]
        if n == 0:
            continue
        bx, sc, lb = boxes[b, :n].clone(), scores[b, :n], labels[b, :n].long()
        f = torch.ones(n, dtype=torch.float32)
        if len(fac) == 1:
            f[:] = fac[0]
        elif fac:
            inside = (lb >= 0) & (lb < len(fac))
            f[inside] = torch.tensor(fac, dtype=torch.float32)[lb[inside]]
        scaled = bx[:, 3:6] * f[:, None]
        order = torch.sort(sc + 0.0, descending=True, stable=True).indices[:pre]
        if nms_type == "rotate":
            q = torch.stack([bx[:, 0], bx[:, 1], scaled[:, 0], scaled[:, 1], bx[:, 6]], 1)[order]
            sup = bev_iou_fp64(q, q) > float(thr32)          # (NaN compares false)
        else:
            x, y = bx[order, 0], bx[order, 1]
            dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
            sup = (dx * dx + dy * dy) <= thr32
        keep = _greedy_keep(order, lambda i: sup[i, i + 1:], post)
        k = keep.numel()
        if fac:
            bx[:, 3:6] = scaled / f[:, None]
        kept = bx[keep]
        if bottom_center:
            kept[:, 2] = kept[:, 2] - kept[:, 5] * 0.5
        out_b[b, :k], out_s[b, :k], out_l[b, :k] = kept, sc[keep], lb[keep].to(torch.int32)
        out_i[b, :k], out_c[b] = keep.to(torch.int32), k
    return out_b, out_s, out_l, out_c, out_i


# ---------------------------------------------------------------------------------------------------------------------
# The 2-D heads: CenterNet, YOLOX and the axis-aligned batched NMS (functions/decode2d.py, csrc/decode2d.hip).  Written
# from the published algorithm of mmdet 2.x (CenterNetHead.get_bboxes / decode_heatmap, YOLOXHead.get_bboxes /
# _bbox_decode / _bboxes_nms) and mmcv.ops.batched_nms, as the reference's detectors call them
# (det2trt/models/detector/{centernet,yolox}.py: post_process); parity with the libraries themselves is unpinned.
def centernet_decode_torch(heatmap, wh, offset, k, input_shape, kernel=3, border=None, scale_factor=None,
                           score_threshold=None, return_index=False):
    """The padded result of `centernet_decode` -- boxes [B, k, 4], scores [B, k], labels int32, count [B] -- in torch ops
    on the CPU: max_pool2d thinning (-inf padding, hmax == heat, a kept -0 as +0), stable descending sort, the box
    arithmetic one fp32 tensor op per step.  Defined for maps without NaN."""
    heat, wh, off = (t.detach().float().cpu() for t in (heatmap, wh, offset))
    B, C, H, W = heat.shape
    k = int(k)
    if not 1 <= k <= C * H * W:
        raise ValueError(f"k {k} outside 1 .. {C * H * W}")
    if kernel < 1 or kernel % 2 == 0:
        raise ValueError(f"kernel {kernel} must be odd")
    hmax = torch.nn.functional.max_pool2d(heat, kernel, stride=1, padding=(kernel - 1) // 2)
    thin = torch.where(hmax == heat, heat, torch.zeros_like(heat)) + 0.0
    flat = thin.reshape(B, -1)
    index = _rank(flat, k)
    scores = torch.gather(flat, 1, index)
    labels = torch.div(index, H * W, rounding_mode="trunc")
    cell = index % (H * W)
    ys, xs = torch.div(cell, W, rounding_mode="trunc").float(), (cell % W).float()
    at = lambda t: torch.gather(t.reshape(B, 2, H * W), 2, cell[:, None, :].expand(B, 2, k))
    w, o = at(wh), at(off)
    xs, ys = xs + o[:, 0], ys + o[:, 1]
    rx = torch.tensor(float(input_shape[1]) / W, dtype=torch.float32)
    ry = torch.tensor(float(input_shape[0]) / H, dtype=torch.float32)
    boxes = torch.stack([(xs - w[:, 0] / 2) * rx, (ys - w[:, 1] / 2) * ry, (xs + w[:, 0] / 2) * rx,
                         (ys + w[:, 1] / 2) * ry], dim=-1)
    bd, sf = _rows(border, B, 2, "border"), _rows(scale_factor, B, 4, "scale_factor")
    if bd is not None:
        boxes = boxes - bd[:, None, [0, 1, 0, 1]]
    if sf is not None:
        boxes = boxes / sf[:, None, :]
    keep = torch.ones(B, k, dtype=torch.bool)
    if score_threshold is not None and score_threshold >= 0:
        keep = scores > score_threshold
    out_b, out_s = torch.zeros(B, k, 4), torch.zeros(B, k)
    out_l, count = torch.zeros(B, k, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        n = int(keep[b].sum())
        out_b[b, :n], out_s[b, :n], out_l[b, :n] = boxes[b][keep[b]], scores[b][keep[b]], labels[b][keep[b]].to(torch.int32)
        count[b] = n
    out = (out_b, out_s, out_l, count)
    return out + (index, keep) if return_index else out


def yolox_decode_torch(cls_scores, bbox_preds, objectnesses, strides=(8, 16, 32), scale_factor=None):
    """The result of `yolox_decode` -- boxes [B, P, 4], scores [B, P], labels [B, P] int32 in prior order -- in torch
    ops on the CPU.  The label is the first maximum of the class LOGITS (the one stated deviation from mmdet, which takes
    it after the sigmoid)."""
    boxes, scores, labels = [], [], []
    for cls, box, obj, stride in zip(cls_scores, bbox_preds, objectnesses, strides):
        cls, box, obj = (t.detach().float().cpu() for t in (cls, box, obj))
        B, C, H, W = cls.shape
        cls = cls.permute(0, 2, 3, 1).reshape(B, H * W, C)
        p = box.permute(0, 2, 3, 1).reshape(B, H * W, 4)
        obj = obj.reshape(B, H * W)
        px = (torch.arange(W) * int(stride)).float().repeat(H)
        py = (torch.arange(H) * int(stride)).float().repeat_interleave(W)
        s = float(stride)
        cx, cy = p[..., 0] * s + px, p[..., 1] * s + py
        w, h = p[..., 2].exp() * s, p[..., 3].exp() * s
        boxes.append(torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], dim=-1))
        best = cls.max(dim=-1).values
        first = torch.where(cls == best[..., None], torch.arange(C).expand_as(cls), torch.full_like(cls, C, dtype=torch.long))
        labels.append(first.min(dim=-1).values.to(torch.int32))
        scores.append(obj.sigmoid() * best.sigmoid())
    boxes, scores, labels = torch.cat(boxes, 1), torch.cat(scores, 1), torch.cat(labels, 1)
    sf = _rows(scale_factor, boxes.shape[0], 4, "scale_factor")
    if sf is not None:
        boxes = boxes / sf[:, None, :]
    return boxes, scores, labels


def box_nms_torch(boxes, scores, labels, count=None, *, score_threshold=None, iou_threshold, class_aware=True,
                  max_out=None):
    """The padded result of `box_nms` -- (boxes [B, max_out, 4], scores, labels int32, count, index int32) -- in torch
    ops on the CPU: candidates score >= score_threshold below count, stable descending sort (equal scores: lower row
    first), the fp32 pair test in the stated operation order, greedy scan, cut to max_out.  The label test is the
    definition of class-awareness (mmcv's coordinate offset is not restated); a row with a non-finite coordinate
    suppresses nothing and is not suppressed."""
    boxes, scores = boxes.detach().float().cpu(), scores.detach().float().cpu()
    labels = labels.detach().cpu()
    if boxes.ndim == 2:
        boxes, scores, labels = boxes[None], scores[None], labels[None]
        count = None if count is None else count.reshape(1)
    B, N = scores.shape
    post = N if max_out is None else int(max_out)
    if not 1 <= post <= N:
        raise ValueError(f"max_out {post} outside 1 .. {N}")
    thr = float("-inf") if score_threshold is None else float(score_threshold)
    iou_thr = torch.tensor(float(iou_threshold), dtype=torch.float32)
    counts = [N] * B if count is None else [min(max(int(c), 0), N) for c in count.tolist()]
    out_b, out_s = torch.zeros(B, post, 4), torch.zeros(B, post)
    out_l, out_i = torch.zeros(B, post, dtype=torch.int32), torch.zeros(B, post, dtype=torch.int32)
    out_c = torch.zeros(B, dtype=torch.int32)
    nan = torch.tensor(float("nan"))
    for b in range(B):
        n = counts[b]
        sc = scores[b, :n]
        rows = torch.nonzero(sc >= thr).flatten()
        if rows.numel() == 0:
            continue
        order = rows[torch.sort(sc[rows] + 0.0, descending=True, stable=True).indices]
        q, lb = boxes[b][order], labels[b][order].long()
        x1, y1, x2, y2 = q.unbind(-1)
        area = torch.where(torch.isfinite(q).all(-1), (x2 - x1) * (y2 - y1), nan)

        def suppressed_by(i):          # row i's pair tests, only once it is kept: never the whole M x M matrix
            iw = (torch.minimum(x2[i], x2[i + 1:]) - torch.maximum(x1[i], x1[i + 1:])).clamp(min=0)
            ih = (torch.minimum(y2[i], y2[i + 1:]) - torch.maximum(y1[i], y1[i + 1:])).clamp(min=0)
            inter = iw * ih
            sup = inter / ((area[i] + area[i + 1:]) - inter) > iou_thr          # (NaN compares false)
            return sup & (lb[i + 1:] == lb[i]) if class_aware else sup

        kept = _greedy_keep(order, suppressed_by, post)
        m = kept.numel()
        out_b[b, :m], out_s[b, :m], out_l[b, :m] = boxes[b][kept], scores[b][kept], labels[b][kept].to(torch.int32)
        out_i[b, :m], out_c[b] = kept.to(torch.int32), m
    return out_b, out_s, out_l, out_c, out_i


def _meta_rows(img_metas, key, pick=None):
    rows = []
    for meta in img_metas:
        v = [float(x) for x in (meta[key].tolist() if hasattr(meta[key], "tolist") else meta[key])]
        rows.append([v[i] for i in pick] if pick else v)
    return rows


def _single_level(preds):
    if torch.is_tensor(preds):
        return preds
    assert len(preds) == 1, "CenterNet has one output level"
    return preds[0]


def centernet_get_bboxes(center_heatmap_preds, wh_preds, offset_preds, img_metas, rescale=True, topk=100,
                         local_maximum_kernel=3):
    """CenterNetHead.get_bboxes (with_nms=False, the reference's config): the three head outputs (one-level lists, as
    mmdet passes them, or the tensors themselves; the heat map after its sigmoid) and mmdet's img_metas
    (`batch_input_shape`, `border` = (top, bottom, left, right) when the test pipeline padded, `scale_factor`).  Returns
    [(det_bboxes [n, 5] = x1, y1, x2, y2, score, det_labels [n] int64)] per image, n = topk.  Device tensors go to the
    kernels, CPU tensors to the torch statement."""
    from .functions.decode2d import centernet_decode
    heat, wh, off = (_single_level(p) for p in (center_heatmap_preds, wh_preds, offset_preds))
    border = _meta_rows(img_metas, "border", (2, 0)) if "border" in img_metas[0] else None
    scale = _meta_rows(img_metas, "scale_factor") if rescale else None
    boxes, scores, labels, count = centernet_decode(heat, wh, off, topk, img_metas[0]["batch_input_shape"],
                                                    local_maximum_kernel, border, scale, padded=True)
    return [(torch.cat([boxes[b, :n], scores[b, :n, None]], dim=-1), labels[b, :n].to(torch.int64))
            for b, n in enumerate(count.tolist())]


def yolox_get_bboxes(cls_scores, bbox_preds, objectnesses, img_metas, rescale=True, score_thr=0.01, iou_threshold=0.65,
                     strides=(8, 16, 32), max_out=None):
    """YOLOXHead.get_bboxes: decode every prior, rescale (before the NMS, as mmdet does), then the class-aware NMS over
    the rows with score >= score_thr.  Returns [(det_bboxes [n, 5], det_labels [n] int64)] per image in descending score
    order; max_out caps n (None = no cap).  Device tensors go to the kernels, CPU tensors to the torch statements."""
    from .functions.decode2d import box_nms, yolox_decode
    scale = _meta_rows(img_metas, "scale_factor") if rescale else None
    boxes, scores, labels = yolox_decode(cls_scores, bbox_preds, objectnesses, strides, scale)
    kb, ks, kl, count, _ = box_nms(boxes, scores, labels, score_threshold=score_thr, iou_threshold=iou_threshold,
                                   class_aware=True, max_out=max_out, padded=True)
    return [(torch.cat([kb[b, :n], ks[b, :n, None]], dim=-1), kl[b, :n].to(torch.int64))
            for b, n in enumerate(count.tolist())]


def _dicts(padded, columns, label_dtype, device):
    boxes, scores, labels, count = padded
    out = []
    for b, n in enumerate(count.tolist()):
        out.append({"bboxes": boxes[b, :n, :columns].to(device), "scores": scores[b, :n].to(device),
                    "labels": labels[b, :n].to(device=device, dtype=label_dtype)})
    return out


class NMSFreeCoder:
    """nms_free_coder.py:10-36.  `decode` returns, per batch item, {"bboxes" [n, 9], "scores" [n], "labels" [n] int64}
    as the reference does; `decode_padded` returns the fixed-size form without a host synchronisation (device tensors).
    bottom_center=True adds the z -= h / 2 of BEVFormerHead.get_bboxes."""

    def __init__(self, pc_range, voxel_size=None, post_center_range=None, max_num=100, score_threshold=None,
                 num_classes=10):
        self.pc_range, self.voxel_size, self.post_center_range = pc_range, voxel_size, post_center_range
        self.max_num, self.score_threshold, self.num_classes = max_num, score_threshold, num_classes

    def encode(self):
        pass

    def decode_padded(self, cls_scores, bbox_preds, bottom_center=False):
        """cls_scores [B, num_query, num_classes] logits, bbox_preds [B, num_query, 10]."""
        if self.post_center_range is None:
            raise NotImplementedError("only post_center_range is not None is supported (as in the reference)")
        if cls_scores.shape[-1] != self.num_classes:
            raise ValueError(f"cls_scores has {cls_scores.shape[-1]} classes, the coder {self.num_classes}")
        fn = nms_free_decode if cls_scores.is_cuda else nms_free_decode_torch
        kw = {"padded": True} if cls_scores.is_cuda else {}
        return fn(cls_scores, bbox_preds, self.max_num, self.post_center_range, self.score_threshold, bottom_center, **kw)

    def decode_single(self, cls_scores, bbox_preds, bottom_center=False):
        return _dicts(self.decode_padded(cls_scores[None], bbox_preds[None], bottom_center), 9, torch.int64,
                      cls_scores.device)[0]

    def decode(self, preds_dicts, bottom_center=False):
        """preds_dicts: {"all_cls_scores" [nb_dec, B, num_query, num_classes], "all_bbox_preds" [nb_dec, B, num_query,
        10]}; the last decoder level is decoded."""
        cls, box = preds_dicts["all_cls_scores"][-1], preds_dicts["all_bbox_preds"][-1]
        return _dicts(self.decode_padded(cls, box, bottom_center), 9, torch.int64, cls.device)


class CenterPointBBoxCoder:
    """centerpoint_bbox_coders.py:9-43.  `decode` has the reference's signature: `heat` holds SCORES (the head applies
    the sigmoid first), `dim` is used as given, the rotation comes as two one-channel maps; labels come back as
    float32, as there.  `decode_heads` takes the six raw maps of BEVDet.forward instead (logits, log sizes with
    norm_bbox) -- CenterHead.get_bboxes up to the NMS -- and returns the padded form."""

    def __init__(self, pc_range, out_size_factor, voxel_size, post_center_range=None, max_num=100, score_threshold=None,
                 code_size=9):
        self.pc_range, self.out_size_factor, self.voxel_size = pc_range, out_size_factor, voxel_size
        self.post_center_range, self.max_num, self.score_threshold = post_center_range, max_num, score_threshold
        self.code_size = code_size

    def encode(self):
        pass

    def _run(self, reg, height, dim, rot, vel, heat, norm_bbox, heatmap_is_score):
        if self.post_center_range is None:
            raise NotImplementedError("only post_center_range is not None is supported (as in the reference)")
        args = (reg, height, dim, rot, vel, heat, self.max_num, self.post_center_range, self.pc_range,
                self.out_size_factor, self.voxel_size, self.score_threshold, norm_bbox, heatmap_is_score)
        return centerpoint_decode(*args, padded=True) if heat.is_cuda else centerpoint_decode_torch(*args)

    def decode_heads(self, reg, height, dim, rot, vel, heatmap, norm_bbox=True):
        return self._run(reg, height, dim, rot, vel, heatmap, norm_bbox, False)

    def decode(self, heat, rot_sine, rot_cosine, hei, dim, vel, reg=None, task_id=-1):
        rot = torch.cat([rot_sine, rot_cosine], dim=1)
        padded = self._run(reg, hei, dim, rot, vel, heat, False, True)
        return _dicts(padded, 9 if vel is not None else 7, torch.float32, heat.device)
