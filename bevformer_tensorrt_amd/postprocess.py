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
reference are cut from it.  Not here: BEVDet's rotated scale-NMS (CenterHead.get_task_detections); `decode` hands back
what that NMS consumes.
"""
import torch

from .functions.decode import nms_free_decode, centerpoint_decode


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
