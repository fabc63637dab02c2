"""Shared by tests/golden/make_decode2d_golden.py and tests/test_decode2d_{cpu,gpu}.py: an independent numpy / float32
statement of the three 2-D post-processing algorithms (CenterNet decode, YOLOX decode, axis-aligned batched NMS) in the
operation order include/bevops.h fixes, float64 values of the transcendental columns, the conditions a fixture must meet
so that a comparison cannot hide a failure, and the loader of tests/golden/decode2d.npz.

Nothing here imports bevformer_tensorrt_amd: the package's torch statements (postprocess.py) and its kernels are what is
compared WITH this file.  float32 arrays combined with float32 scalars round every operation once, like the kernels'
*_rn helpers and like one torch tensor op per step."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode2d.npz")
F32 = np.float32

# Transcendental columns of the YOLOX decode (corners through exp, score through two sigmoids): error against the
# float64 value, measured on the fixtures (design/postprocess.md, "2-D heads: measured errors").  The bar is twice the
# larger of the two measured maxima, rounded up to a whole ulp.
#   corners: unit = ulp32(larger |corner| of the box along that axis); score: unit = ulp32(score)
MEASURED_ULP = {"corner": {"torch_cpu": 1.4782, "kernel": 1.4782}, "score": {"torch_cpu": 2.3075, "kernel": 2.2906}}
BAR_ULP = {"corner": 3, "score": 5}      # ceil(2 * 1.4782), ceil(2 * 2.3075)

REL_GAP = 1e-5       # scores: distance from the threshold and from each other, relative
LOGIT_GAP = 1e-3     # top two class logits of a prior
LOGIT_MAX = 12.0
IOU_BAND = 1e-3      # float64 IoU of a candidate pair to the threshold


def ulp32(x):
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return 2.0 ** (np.maximum(e, -126) - 23)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------- CenterNet
def np_centernet(heat, wh, off, k, kernel, inp, border=None, scale=None, thr=None):
    """heat [B, C, H, W], wh / off [B, 2, H, W] (any float dtype, widened); inp = (inp_h, inp_w); border [B, 2] =
    (x, y) or None; scale [B, 4] or None; thr None / < 0 = no score test.  Returns the padded form and the selected
    flat indices: boxes [B, k, 4], scores [B, k], labels [B, k] int32, count [B] int32, index [B, k] int64."""
    heat, wh, off = (np.asarray(a).astype(F32) for a in (heat, wh, off))
    B, C, H, W = heat.shape
    r = (kernel - 1) // 2
    pad = np.full((B, C, H + 2 * r, W + 2 * r), -np.inf, F32)
    pad[..., r:r + H, r:r + W] = heat
    hmax = np.full_like(heat, -np.inf)
    for dy in range(kernel):
        for dx in range(kernel):
            hmax = np.maximum(hmax, pad[..., dy:dy + H, dx:dx + W])
    thin = np.where(hmax == heat, heat, F32(0)) + F32(0)          # (+ 0: a kept -0 counts as +0)
    rx, ry = F32(float(inp[1]) / W), F32(float(inp[0]) / H)
    boxes, scores = np.zeros((B, k, 4), F32), np.zeros((B, k), F32)
    labels, count = np.zeros((B, k), np.int32), np.zeros(B, np.int32)
    index = np.zeros((B, k), np.int64)
    half = F32(2)
    for b in range(B):
        flat = thin[b].reshape(-1)
        order = np.argsort(-flat.astype(np.float64), kind="stable")[:k]
        index[b] = order
        cell = order % (H * W)
        x, y = (cell % W).astype(F32), (cell // W).astype(F32)
        w0, w1 = wh[b, 0].reshape(-1)[cell], wh[b, 1].reshape(-1)[cell]
        xs, ys = x + off[b, 0].reshape(-1)[cell], y + off[b, 1].reshape(-1)[cell]
        cols = [(xs - w0 / half) * rx, (ys - w1 / half) * ry, (xs + w0 / half) * rx, (ys + w1 / half) * ry]
        if border is not None:
            cols = [c - F32(border[b][i & 1]) for i, c in enumerate(cols)]
        if scale is not None:
            cols = [c / F32(scale[b][i]) for i, c in enumerate(cols)]
        bx, sc, lb = np.stack(cols, -1).astype(F32), flat[order], (order // (H * W)).astype(np.int32)
        keep = np.ones(k, bool) if thr is None or thr < 0 else sc > F32(thr)
        n = int(keep.sum())
        boxes[b, :n], scores[b, :n], labels[b, :n], count[b] = bx[keep], sc[keep], lb[keep], n
    return boxes, scores, labels, count, index


# ------------------------------------------------------------------------------------------------------- YOLOX
def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def np_yolox(cls_list, box_list, obj_list, strides, scale=None):
    """Per level cls [B, C, H, W], box [B, 4, H, W], obj [B, 1, H, W] logits.  Returns a dict: the float32 statement
    (`boxes`, `scores`, `labels`), the float64 values of the same columns (`boxes64`, `scores64`) and `exact`: the
    priors whose log sizes are both 0, so that w = h = stride exactly and their corners involve no transcendental."""
    out = {k: [] for k in ("boxes", "scores", "labels", "boxes64", "scores64", "exact", "top2")}
    for cls, box, obj, stride in zip(cls_list, box_list, obj_list, strides):
        cls, box, obj = (np.asarray(a).astype(F32) for a in (cls, box, obj))
        B, C, H, W = cls.shape
        cls = cls.transpose(0, 2, 3, 1).reshape(B, H * W, C)
        p = box.transpose(0, 2, 3, 1).reshape(B, H * W, 4)
        obj = obj.reshape(B, H * W)
        px = np.tile(np.arange(W) * stride, H).astype(F32)
        py = np.repeat(np.arange(H) * stride, W).astype(F32)
        s = F32(stride)
        for dt, key_b, key_s in ((F32, "boxes", "scores"), (np.float64, "boxes64", "scores64")):
            q, two = p.astype(dt), dt(2)
            cx, cy = q[..., 0] * dt(s) + px.astype(dt), q[..., 1] * dt(s) + py.astype(dt)
            w, h = np.exp(q[..., 2]) * dt(s), np.exp(q[..., 3]) * dt(s)
            out[key_b].append(np.stack([cx - w / two, cy - h / two, cx + w / two, cy + h / two], -1).astype(dt))
            out[key_s].append((_sigmoid(obj.astype(dt)) * _sigmoid(cls.max(-1).astype(dt))).astype(dt))
        out["labels"].append(cls.argmax(-1).astype(np.int32))            # first maximum
        out["exact"].append((p[..., 2] == 0) & (p[..., 3] == 0))
        srt = np.sort(cls, -1)
        out["top2"].append(srt[..., -1] - srt[..., -2] if C > 1 else np.full(obj.shape, np.inf, F32))
    out = {k: np.concatenate(v, 1) for k, v in out.items()}
    if scale is not None:
        sf = np.asarray(scale, F32).reshape(-1, 1, 4)
        out["boxes"] = (out["boxes"] / sf).astype(F32)
        out["boxes64"] = out["boxes64"] / sf.astype(np.float64)
    return out


# ------------------------------------------------------------------------------------------------------- box NMS
def iou_matrix(boxes, dtype):
    """IoU [n, n] of boxes [n, 4] in the stated operation order, evaluated in `dtype`."""
    b = np.asarray(boxes).astype(dtype)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    zero = dtype(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        area = (x2 - x1) * (y2 - y1)
        iw = np.maximum(np.minimum(x2[:, None], x2[None, :]) - np.maximum(x1[:, None], x1[None, :]), zero)
        ih = np.maximum(np.minimum(y2[:, None], y2[None, :]) - np.maximum(y1[:, None], y1[None, :]), zero)
        inter = iw * ih
        return inter / ((area[:, None] + area[None, :]) - inter)


def candidates(scores, count, thr):
    """Candidate rows of one item in rank order: below count, score >= thr; descending score, lower row first."""
    s = np.asarray(scores, F32)[:count]
    rows = np.nonzero(s >= F32(thr))[0]
    return rows[np.argsort(-(s[rows] + F32(0)).astype(np.float64), kind="stable")]


def np_box_nms(boxes, scores, labels, count, thr, iou_thr, aware, max_out):
    """boxes [B, N, 4], scores [B, N], labels [B, N] int32, count [B] or None.  Returns the padded form: boxes
    [B, max_out, 4], scores, labels, count [B], index [B, max_out] int32."""
    boxes, scores, labels = np.asarray(boxes, F32), np.asarray(scores, F32), np.asarray(labels, np.int32)
    B, N = scores.shape
    out_b, out_s = np.zeros((B, max_out, 4), F32), np.zeros((B, max_out), F32)
    out_l, out_i = np.zeros((B, max_out), np.int32), np.zeros((B, max_out), np.int32)
    out_c = np.zeros(B, np.int32)
    for b in range(B):
        n = N if count is None else min(max(int(count[b]), 0), N)
        order = candidates(scores[b], n, thr)
        if order.size == 0:
            continue
        iou = iou_matrix(boxes[b][order], F32)
        finite = np.isfinite(boxes[b][order]).all(-1)
        sup = (iou > F32(iou_thr)) & finite[:, None] & finite[None, :]
        if aware:
            sup &= labels[b][order][:, None] == labels[b][order][None, :]
        removed, keep = np.zeros(order.size, bool), []
        for i in range(order.size):
            if removed[i]:
                continue
            keep.append(i)
            if len(keep) == max_out:
                break
            removed[i + 1:] |= sup[i, i + 1:]
        kept = order[keep]
        m = kept.size
        out_b[b, :m], out_s[b, :m], out_l[b, :m] = boxes[b][kept], scores[b][kept], labels[b][kept]
        out_i[b, :m], out_c[b] = kept, m
    return out_b, out_s, out_l, out_c, out_i


# ------------------------------------------------------------------------------------------------------- conditions
def check_scores(scores64, thr, what):
    """No score within REL_GAP (relative) of the threshold; no two candidate scores closer than REL_GAP (relative)."""
    s = np.asarray(scores64, np.float64)
    assert (np.abs(s - thr) > REL_GAP * thr).all(), f"{what}: a score within {REL_GAP} of the threshold"
    c = np.sort(s[s >= thr])
    if c.size > 1:
        assert (np.diff(c) > REL_GAP * c[1:]).all(), f"{what}: two candidate scores closer than {REL_GAP}"


def check_logits(cls_list, top2, what):
    for cls in cls_list:
        assert np.abs(np.asarray(cls, np.float64)).max() <= LOGIT_MAX, f"{what}: |logit| above {LOGIT_MAX}"
    assert (np.asarray(top2) >= LOGIT_GAP).all(), f"{what}: top two class logits closer than {LOGIT_GAP}"


def check_iou_band(boxes64, cand, iou_thr, what, labels=None):
    """No candidate pair (same label only, when labels are given) has a float64 IoU within IOU_BAND of the threshold."""
    iou = iou_matrix(np.asarray(boxes64, np.float64)[cand], np.float64)
    pair = np.triu(np.ones_like(iou, bool), 1)
    if labels is not None:
        lb = np.asarray(labels)[cand]
        pair &= lb[:, None] == lb[None, :]
    near = pair & (np.abs(iou - iou_thr) < IOU_BAND)
    assert not near.any(), f"{what}: a pair's IoU within {IOU_BAND} of the threshold"


# ------------------------------------------------------------------------------------------------------- loader
_DATA = None


def data():
    global _DATA
    if _DATA is None:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _DATA = {k: z[k] for k in z.files}
    return _DATA


def _opt(d, key):
    return d[key] if key in d else None


def cn_cases():
    d = data()
    out = []
    for name in d["cn_names"]:
        name = str(name)
        g = lambda k: d[f"{name}_{k}"]
        k, kernel, inp_h, inp_w, f16 = (int(v) for v in g("params"))
        out.append(dict(name=name, heat=g("heat").astype(F32), wh=g("wh").astype(F32), off=g("off").astype(F32), k=k,
                        kernel=kernel, inp=(inp_h, inp_w), f16=bool(f16), border=_opt(d, f"{name}_border"),
                        scale=_opt(d, f"{name}_scale"), boxes=g("boxes"), scores=g("scores"), labels=g("labels"),
                        count=g("count"), index=g("index")))
    return out


def yx_cases():
    d = data()
    out = []
    for name in d["yx_names"]:
        name = str(name)
        g = lambda k: d[f"{name}_{k}"]
        L = int(g("levels").shape[0])
        out.append(dict(name=name, levels=g("levels"), strides=[int(s) for s in g("levels")[:, 2]],
                        cls=[g(f"cls{l}") for l in range(L)], box=[g(f"box{l}") for l in range(L)],
                        obj=[g(f"obj{l}") for l in range(L)], scale=_opt(d, f"{name}_scale"),
                        score_thr=float(g("params")[0]), iou_thr=float(g("params")[1]), max_out=int(g("params")[2]),
                        boxes=g("boxes"), scores=g("scores"), labels=g("labels"), boxes64=g("boxes64"),
                        scores64=g("scores64"), exact=g("exact"), top2=g("top2"),
                        nms={a: tuple(g(f"nms{a}_{k}") for k in ("boxes", "scores", "labels", "count", "index"))
                             for a in (0, 1)}))
    return out


def nm_cases():
    d = data()
    out = []
    for name in d["nm_names"]:
        name = str(name)
        g = lambda k: d[f"{name}_{k}"]
        thr, iou_thr, aware, max_out = g("params")
        out.append(dict(name=name, boxes=g("in_boxes"), scores=g("in_scores"), labels=g("in_labels"),
                        count=_opt(d, f"{name}_in_count"), score_thr=float(thr), iou_thr=float(iou_thr), aware=int(aware),
                        max_out=int(max_out), want=tuple(g(k) for k in ("boxes", "scores", "labels", "count", "index"))))
    return out


def yx_levels(case, dtype=None, device=None, channels_last=False):
    """The level tensors of a YOLOX case as torch tensors: (cls list, box list, obj list)."""
    import torch

    def t(a):
        x = torch.from_numpy(np.ascontiguousarray(a))
        x = x if dtype is None else x.to(dtype)
        x = x if device is None else x.to(device)
        return x.contiguous(memory_format=torch.channels_last) if channels_last else x
    return [t(a) for a in case["cls"]], [t(a) for a in case["box"]], [t(a) for a in case["obj"]]


def yolox_errors(boxes, scores, case):
    """(corner, score): the largest error of a YOLOX decode against the case's float64 values, in ulp.  Corners: the
    unit is one float32 ulp of the larger |corner| of that box along the axis (the magnitude of cx +- w / 2's operands:
    the difference cannot be better than the roundings of its terms); score: one ulp of the score."""
    b, s = np.asarray(boxes, np.float64), np.asarray(scores, np.float64)
    t = case["boxes64"]
    unit = np.empty_like(t)
    for lo, hi in ((0, 2), (1, 3)):
        unit[..., lo] = unit[..., hi] = ulp32(np.maximum(np.abs(t[..., lo]), np.abs(t[..., hi])))
    return float((np.abs(b - t) / unit).max()), float((np.abs(s - case["scores64"]) / ulp32(case["scores64"])).max())
