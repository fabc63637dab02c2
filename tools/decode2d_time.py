#!/usr/bin/env python3
"""The 2-D heads' post-processing (csrc/decode2d.hip) timed under HIP-graph replay at the reference's shapes, against
the same steps written as torch device ops on the same GPU:
  centernet  bevops_centernet_decode, 80 x 128 x 128, k = 100, kernel 3, border + rescale, fp32 and fp16 channels-last,
             against mmdet's decode_heatmap as torch ops (max_pool2d, ==, topk, gathers, box arithmetic): all of it has
             fixed shapes and is captured;
  yolox      bevops_yolox_decode, 3 levels at 640 x 640 (8 400 priors) x 80 classes, against the torch statement of
             _bbox_decode + score + label (cat, exp, sigmoid, max): all of it is captured;
  box_nms    bevops_box_nms on those 8 400 decoded rows at score_thr 0.01, IoU 0.65, class-aware, against the CAPTURABLE
             part of the same steps as torch ops -- the score mask, the descending sort, the 8 400 x 8 400 IoU matrix and
             its comparison with the threshold and the labels.  NOT captured, and not in the torch number: the boolean-mask
             indexing (a data-dependent shape) and the greedy scan over the matrix, which has no torch-op form without a
             host loop (mmcv runs its own kernel and copies the mask to the host).
Per step: the median and the max over >= 7 rounds of one replay of `iters` captured calls.  One JSON line per row, also
appended to --out (default profiles/decode2d/decode2d_time.jsonl).

    python tools/decode2d_time.py [--rounds 7] [--out FILE]      every step in a fresh child process under `timeout`;
                                                                 stops at the first step that fails
    python tools/decode2d_time.py --step NAME [--rounds 7]       one step in this process
    python tools/decode2d_time.py --once                         every entry once, eagerly, no timing (for a
                                                                 `rocprofv3 --kernel-trace --stats -- python ...` run:
                                                                 launches per call)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"centernet": 240, "yolox": 240, "box_nms": 300}      # seconds allowed per step
ITERS = 20


def graph_times_us(fn, iters, rounds):
    """Per-call microseconds of `iters` captured calls, one number per replay round."""
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return out


def stats(ts):
    return {"median": round(statistics.median(ts), 2), "max": round(max(ts), 2), "rounds": len(ts)}


def centernet_inputs(dtype, channels_last):
    import torch
    g = torch.Generator().manual_seed(0)
    heat = torch.sigmoid(torch.randn(1, 80, 128, 128, generator=g) * 1.5 - 3.0)
    wh, off = torch.rand(1, 2, 128, 128, generator=g) * 20, torch.rand(1, 2, 128, 128, generator=g)
    to = lambda t: t.to("cuda", dtype).contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    return to(heat), to(wh), to(off)


def centernet_torch(heat, wh, off, k, inp, border, scale):
    """mmdet's decode_heatmap + border + rescale as torch device ops (B = 1)."""
    import torch
    import torch.nn.functional as F
    B, C, H, W = heat.shape
    hmax = F.max_pool2d(heat, 3, stride=1, padding=1)
    thin = heat * (hmax == heat).to(heat.dtype)
    scores, index = torch.topk(thin.reshape(B, -1), k)
    labels = index // (H * W)
    cell = index % (H * W)
    ys, xs = (cell // W).float(), (cell % W).float()
    at = lambda t: torch.gather(t.reshape(B, 2, H * W).float(), 2, cell[:, None, :].expand(B, 2, k))
    w, o = at(wh), at(off)
    xs, ys = xs + o[:, 0], ys + o[:, 1]
    rx, ry = inp[1] / W, inp[0] / H
    boxes = torch.stack([(xs - w[:, 0] / 2) * rx, (ys - w[:, 1] / 2) * ry, (xs + w[:, 0] / 2) * rx,
                         (ys + w[:, 1] / 2) * ry], dim=-1)
    return (boxes - border) / scale, scores, labels


def yolox_inputs(dtype, channels_last, obj_shift=-2.5):
    import torch
    g = torch.Generator().manual_seed(1)
    shapes = [(80, 80), (40, 40), (20, 20)]
    to = lambda t: t.to("cuda", dtype).contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    cls = [torch.randn(1, 80, h, w, generator=g) * 2 for h, w in shapes]
    for c in cls:
        c[:, :3] += 4.0          # three classes dominate, so that same-label neighbours meet in the NMS
    cls = [to(c) for c in cls]
    box = [to(torch.cat([torch.randn(1, 2, h, w, generator=g), torch.randn(1, 2, h, w, generator=g) * 0.3 + 1.9], 1))
           for h, w in shapes]
    obj = [to(torch.randn(1, 1, h, w, generator=g) * 2.5 + obj_shift) for h, w in shapes]
    return cls, box, obj


def yolox_torch(cls, box, obj, strides, scale, priors):
    import torch
    B = cls[0].shape[0]
    flat = lambda ts, c: torch.cat([t.permute(0, 2, 3, 1).reshape(B, -1, c) for t in ts], 1).float()
    c, p, o = flat(cls, cls[0].shape[1]), flat(box, 4), flat(obj, 1)[..., 0]
    xy = p[..., :2] * priors[:, 2:] + priors[:, :2]
    half = p[..., 2:].exp() * priors[:, 2:] / 2
    boxes = torch.cat([xy - half, xy + half], -1) / scale
    best, labels = c.max(-1)
    return boxes, o.sigmoid() * best.sigmoid(), labels


def nms_torch_capturable(boxes, scores, labels, score_thr, iou_thr):
    """Score mask, descending sort, IoU matrix, threshold and label comparison (B = 1): the part with fixed shapes."""
    import torch
    s = torch.where(scores >= score_thr, scores, torch.full_like(scores, -1.0))
    order = torch.sort(s[0], descending=True, stable=True).indices
    b, lb = boxes[0][order], labels[0][order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = (torch.minimum(b[:, None, 2], b[None, :, 2]) - torch.maximum(b[:, None, 0], b[None, :, 0])).clamp(min=0)
    ih = (torch.minimum(b[:, None, 3], b[None, :, 3]) - torch.maximum(b[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = iw * ih
    iou = inter / (area[:, None] + area[None, :] - inter)
    return (iou > iou_thr) & (lb[:, None] == lb[None, :])


def step(name, rounds, once):
    import torch
    sys.path.insert(0, ROOT)
    import bevformer_tensorrt_amd as bev
    rows = []
    if name == "centernet":
        border_h, scale_h = [[2.0, 6.0]], [[1.6, 1.5, 1.6, 1.5]]
        border = torch.tensor([2.0, 6.0, 2.0, 6.0], device="cuda")
        scale = torch.tensor(scale_h[0], device="cuda")
        for dtype, cl in ((torch.float32, False), (torch.float16, True)):
            heat, wh, off = centernet_inputs(dtype, cl)
            ours = lambda: bev.centernet_decode(heat, wh, off, 100, (512, 512), 3, border_h, scale_h, padded=True)
            if once:
                ours()
                continue
            rows.append({"op": "centernet_decode", "dtype": str(dtype).split(".")[-1], "channels_last": cl,
                         "shape": [1, 80, 128, 128], "k": 100, "iters": ITERS, "us": stats(graph_times_us(ours, ITERS, rounds)),
                         "torch_ops_us": stats(graph_times_us(lambda: centernet_torch(heat, wh, off, 100, (512, 512), border,
                                                                                      scale), ITERS, rounds)),
                         "torch_part": "all of decode_heatmap + border + rescale (captured)"})
    elif name in ("yolox", "box_nms"):
        scale_h = [[1.6, 1.5, 1.6, 1.5]]
        scale = torch.tensor(scale_h[0], device="cuda")
        pri = []
        for (h, w), s in zip([(80, 80), (40, 40), (20, 20)], (8, 16, 32)):
            yy, xx = torch.meshgrid(torch.arange(h) * s, torch.arange(w) * s, indexing="ij")
            pri.append(torch.stack([xx.reshape(-1), yy.reshape(-1), torch.full((h * w,), s), torch.full((h * w,), s)], -1))
        priors = torch.cat(pri).float().cuda()
        for dtype, cl in ((torch.float32, False), (torch.float16, True)):
            cls, box, obj = yolox_inputs(dtype, cl)
            ours = lambda: bev.yolox_decode(cls, box, obj, (8, 16, 32), scale_h)
            if name == "yolox":
                if once:
                    ours()
                    continue
                rows.append({"op": "yolox_decode", "dtype": str(dtype).split(".")[-1], "channels_last": cl, "priors": 8400,
                             "classes": 80, "iters": ITERS, "us": stats(graph_times_us(ours, ITERS, rounds)),
                             "torch_ops_us": stats(graph_times_us(lambda: yolox_torch(cls, box, obj, (8, 16, 32), scale,
                                                                                      priors), ITERS, rounds)),
                             "torch_part": "all of _bbox_decode + score + label (captured)"})
                continue
            if dtype != torch.float32:
                continue
            # two loads: most rows above score_thr (objectness logits around -2.5), and few (around -9)
            for load, shift in (("dense", -2.5), ("sparse", -9.0)):
                boxes, scores, labels = bev.yolox_decode(*yolox_inputs(dtype, cl, shift), (8, 16, 32), scale_h)
                nms = lambda: bev.box_nms(boxes, scores, labels, score_threshold=0.01, iou_threshold=0.65, padded=True)
                if once:
                    if load == "dense":
                        nms()
                    continue
                out = nms()
                rows.append({"op": "box_nms", "load": load, "rows": 8400, "candidates": int((scores >= 0.01).sum()),
                             "kept": int(out[3][0]), "score_thr": 0.01, "iou_thr": 0.65, "iters": ITERS,
                             "us": stats(graph_times_us(nms, ITERS, rounds)),
                             "torch_ops_us": stats(graph_times_us(lambda: nms_torch_capturable(boxes, scores, labels, 0.01,
                                                                                               0.65), 4, rounds)),
                             "torch_part": "score mask + sort + 8400 x 8400 IoU matrix + threshold and label comparison "
                                           "(captured); boolean-mask indexing and the greedy scan are NOT included"})
    else:
        raise SystemExit(f"unknown step {name}")
    torch.cuda.synchronize()
    for r in rows:
        print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode2d", "decode2d_time.jsonl"))
    args = ap.parse_args()
    if args.rounds < 7 and not args.once:
        raise SystemExit("--rounds must be at least 7")
    if args.once:
        for name in STEPS:
            step(name, args.rounds, True)
        return
    if args.step:
        step(args.step, args.rounds, False)
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as out:
        for name, limit in STEPS.items():      # a fresh process per step, each under its own time limit
            res = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
                                  "--rounds", str(args.rounds)], stdout=subprocess.PIPE, text=True)
            sys.stdout.write(res.stdout)
            out.write(res.stdout)
            out.flush()
            if res.returncode != 0:
                raise SystemExit(f"step {name} ended with status {res.returncode}: stopping")


if __name__ == "__main__":
    main()
