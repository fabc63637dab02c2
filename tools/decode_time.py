#!/usr/bin/env python3
"""The detection decode (csrc/decode.hip) timed under HIP-graph replay against the torch op sequence of the reference's
coders on the same device tensors, at BEVFormer-base's shape (900 x 10 logits, top 300) and BEVDet-R50's
(10 x 128 x 128 heat map, top 500, threshold 0.1), fp16 (as the models emit; the torch sequence widens first, as
`force_fp32` does) and fp32.

The torch sequence is timed in two parts, because only the first can be captured:
  torch_graph_us   sigmoid, topk, index arithmetic, gathers, exp, atan2, concatenation, range / score masks -- everything
                   up to the masks, under graph replay like ours;
  torch_mask_index_eager_us   the boolean-mask indexing that produces the trimmed boxes / scores / labels: data-dependent
                   shapes, a host synchronisation each, so it is timed EAGERLY with a host clock around a synchronise
                   (not comparable one-to-one with a replayed number: it includes launch overhead; ours has no
                   counterpart, the padded outputs need no such step).
Per case: median and max over >= 5 rounds of one replay of `iters` calls each.  One JSON line per case.
    python tools/decode_time.py [--rounds 7] [--once]
    python tools/decode_time.py --frame-ab tiny base [--pairs 3]
    python tools/decode_time.py --nms [--rounds 7] [--once]
    python tools/decode_time.py --bevdet-ab [--pairs 3]
--once: every decode once, eagerly, no timing (for a `rocprofv3 --kernel-trace --stats` run: launches per call).
--frame-ab: the whole frame with FrameRunner(decode=True) against decode=False as interleaved same-box pairs, each a
fresh `tools/model_bench.py MODEL --graph --no-clone --static-image --frames 40 [--decode]` process.
--nms: the BEV NMS (csrc/nms.hip) at BEVDet-R50's configuration (500 candidates, threshold 0.2, the per-class rescale
factors, post_max_size 500; circle: min_radius 4, post_max_size 83) on a clustered scene (every object with ~8 near
duplicates, as the top cells of a heat map) and on a sparse one (no overlaps), against the formulation a user without
the kernel would write: the suppression matrix in vectorised torch device ops (rotate: both boxes' corners and edge
intersections, sorted by angle, shoelace -- the usual differentiable rotated-IoU recipe; circle: one broadcast) plus the
greedy loop as 500 row updates, captured and replayed the same way (`torch_graph_us`; the loop alone is
`torch_scan_graph_us`).
--bevdet-ab: the BEVDet-R50 frame (forward + post-processing in one captured graph) with get_bboxes against
get_candidates as interleaved pairs of fresh processes (`--bevdet-frame MODE` is the child)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bevformer_tensorrt_amd as bev  # noqa: E402
from qkv_time import graph_times_us, stats  # noqa: E402

RANGE = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]


def torch_nms_free(cls, box, K, rng):
    """NMSFreeCoder.decode_single's op sequence up to the masks (one batch item), + the z shift of get_bboxes."""
    cls, box = cls.float(), box.float()
    nc = cls.shape[-1]
    scores, index = cls.sigmoid().view(-1).topk(K)
    labels = index % nc
    p = box[torch.div(index, nc, rounding_mode="trunc")]
    boxes = torch.cat([p[:, 0:1], p[:, 1:2], p[:, 4:5], p[:, 2:3].exp(), p[:, 3:4].exp(), p[:, 5:6].exp(),
                       torch.atan2(p[:, 6:7], p[:, 7:8]), p[:, 8:9], p[:, 9:10]], dim=-1)
    mask = (boxes[:, :3] >= rng[:3]).all(1)
    mask &= (boxes[:, :3] <= rng[3:]).all(1)
    return boxes, scores, labels, mask


def torch_centerpoint(reg, hei, dim, rot, vel, heat, K, rng, thr, osf, voxel, pc):
    """CenterHead.get_bboxes + CenterPointBBoxCoder.decode's op sequence up to the masks: sigmoid, exp, top-K per class,
    top-K of those, the (permute, contiguous, gather) of every head, atan2, the affine of x / y, concatenation."""
    reg, hei, dim, rot, vel, heat = (t.float() for t in (reg, hei, dim, rot, vel, heat))
    B, nc, H, W = heat.shape
    heat, dim = heat.sigmoid(), dim.exp()
    s1, i1 = torch.topk(heat.view(B, nc, -1), K)
    i1 = i1 % (H * W)
    ys, xs = (i1.float() / W).int().float(), (i1 % W).int().float()
    scores, i2 = torch.topk(s1.view(B, -1), K)
    labels = (i2 / K).int()
    pick = lambda t: t.view(B, -1, 1).gather(1, i2.unsqueeze(2)).view(B, K)
    cell, ys, xs = pick(i1), pick(ys), pick(xs)

    def at(t):
        t = t.permute(0, 2, 3, 1).contiguous().view(B, H * W, t.shape[1])
        return t.gather(1, cell.unsqueeze(2).expand(B, K, t.shape[2]))
    r = at(reg)
    xs = (xs.view(B, K, 1) + r[:, :, 0:1]) * osf * voxel[0] + pc[0]
    ys = (ys.view(B, K, 1) + r[:, :, 1:2]) * osf * voxel[1] + pc[1]
    rt = at(rot)
    boxes = torch.cat([xs, ys, at(hei), at(dim), torch.atan2(rt[:, :, 0:1], rt[:, :, 1:2]), at(vel)], dim=2)
    mask = (boxes[..., :3] >= rng[:3]).all(2)
    mask &= (boxes[..., :3] <= rng[3:]).all(2)
    mask &= scores > thr
    return boxes, scores, labels.float(), mask


R50_FACTORS = [1.0, 0.7, 0.7, 0.4, 0.55, 1.1, 1.0, 1.0, 1.5, 3.5]      # configs/bevdet/bevdet-r50-cbgs.py:182


_SIGNS = {}


def torch_rotated_iou(q):
    """IoU [n, n] of boxes q [n, 5] (x, y, w, l, yaw) in torch device ops, fixed shapes (capturable): the 8 corners that
    lie inside the other box and the 16 edge-edge intersections, sorted by angle about their mean, shoelace.  (Parallel
    edges give no intersection, so a box against itself -- the diagonal, which the NMS never reads -- comes out 0.)"""
    n = q.shape[0]
    c, s = torch.cos(q[:, 4]), torch.sin(q[:, 4])
    if q.device not in _SIGNS:       # (made by the warm-up call: a host-to-device copy cannot be captured)
        _SIGNS[q.device] = (torch.tensor([0.5, -0.5, -0.5, 0.5], device=q.device),
                            torch.tensor([0.5, 0.5, -0.5, -0.5], device=q.device))
    sx, sy = _SIGNS[q.device]
    lx, ly = q[:, 2:3] * sx, q[:, 3:4] * sy
    corners = torch.stack([q[:, 0:1] + lx * c[:, None] - ly * s[:, None],
                           q[:, 1:2] + lx * s[:, None] + ly * c[:, None]], -1)                # [n, 4, 2]
    A = (corners[:, None] - q[:, None, None, :2]).expand(n, n, 4, 2)                            # relative to box i
    Bc = corners[None] - q[:, None, None, :2]                                                   # box j, same origin

    def inside(pts, ctr, cc, ss, w, l):            # pts [n, n, 4, 2] inside the box (ctr, w, l, yaw) broadcast [n, n]
        d = pts - ctr[:, :, None, :]
        u = d[..., 0] * cc[:, :, None] + d[..., 1] * ss[:, :, None]
        v = d[..., 1] * cc[:, :, None] - d[..., 0] * ss[:, :, None]
        return (u.abs() <= 0.5 * w[:, :, None] + 1e-6) & (v.abs() <= 0.5 * l[:, :, None] + 1e-6)
    zero = torch.zeros(n, n, 2, device=q.device)
    ci, si, wi, li = (t[:, None].expand(n, n) for t in (c, s, q[:, 2], q[:, 3]))
    cj, sj, wj, lj = (t[None, :].expand(n, n) for t in (c, s, q[:, 2], q[:, 3]))
    ctr_j = (q[None, :, :2] - q[:, None, :2])
    a_in_b, b_in_a = inside(A, ctr_j, cj, sj, wj, lj), inside(Bc, zero, ci, si, wi, li)
    a0, a1 = A[:, :, :, None, :], A.roll(-1, 2)[:, :, :, None, :]                               # edges of i x edges of j
    b0, b1 = Bc[:, :, None, :, :], Bc.roll(-1, 2)[:, :, None, :, :]
    da, db = a1 - a0, b1 - b0
    den = da[..., 0] * db[..., 1] - da[..., 1] * db[..., 0]
    w0 = b0 - a0
    t = (w0[..., 0] * db[..., 1] - w0[..., 1] * db[..., 0]) / den
    u = (w0[..., 0] * da[..., 1] - w0[..., 1] * da[..., 0]) / den
    hit = (den.abs() > 1e-12) & (t >= 0) & (t <= 1) & (u >= 0) & (u <= 1)
    cross = (a0 + t[..., None] * da).reshape(n, n, 16, 2)
    pts = torch.cat([A, Bc, cross], 2)                                                          # [n, n, 24, 2]
    ok = torch.cat([a_in_b, b_in_a, hit.reshape(n, n, 16)], 2)
    cnt = ok.sum(2).clamp(min=1)
    mean = (pts * ok[..., None]).sum(2) / cnt[..., None]
    rel = pts - mean[:, :, None, :]
    ang = torch.where(ok, torch.atan2(rel[..., 1], rel[..., 0]), torch.full_like(rel[..., 0], 10.0))
    order = ang.argsort(2)
    rel = rel.gather(2, order[..., None].expand(-1, -1, -1, 2))
    ok = ok.gather(2, order)
    first = rel[:, :, :1]
    nxt = torch.where(ok.roll(-1, 2)[..., None], rel.roll(-1, 2), first.expand_as(rel))        # wrap to the first vertex
    tw = (rel[..., 0] * nxt[..., 1] - nxt[..., 0] * rel[..., 1]) * ok
    inter = 0.5 * tw.sum(2).abs()
    area = q[:, 2] * q[:, 3]
    union = area[:, None] + area[None, :] - inter
    return torch.where(union > 0, inter / union, torch.zeros_like(union))


def torch_nms(boxes, scores, labels, factors, thr, post, circle):
    """What a user of the decoders alone would write on the device: sort, scale, suppression matrix, the greedy loop as
    one row update per candidate (no host round trip, so it can be captured), gather, divide back, z shift.  Returns
    the keep mask in rank order and the restored boxes (the compaction to the front is not even included)."""
    order = scores.argsort(descending=True, stable=True)
    b, l = boxes[order], labels[order].long()
    if circle:
        dx, dy = b[:, None, 0] - b[None, :, 0], b[:, None, 1] - b[None, :, 1]
        sup = (dx * dx + dy * dy) <= thr
        f = None
    else:
        f = factors[l][:, None]
        sized = b[:, 3:6] * f
        sup = torch_rotated_iou(torch.stack([b[:, 0], b[:, 1], sized[:, 0], sized[:, 1], b[:, 6]], 1)) > thr
    sup = sup.triu(1)
    keep = torch_scan(sup, post)
    out = b.clone()
    if f is not None:
        out[:, 3:6] = sized / f
    out[:, 2] = out[:, 2] - out[:, 5] * 0.5
    return keep, out, scores[order], l


def torch_scan(sup, post):
    n = sup.shape[0]
    removed = torch.zeros(n, dtype=torch.bool, device=sup.device)
    for i in range(n):
        removed |= sup[i] & ~removed[i]
    keep = ~removed
    return keep & (keep.cumsum(0) <= post)


def nms_scenes():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import util_nms as U
    rng = np.random.default_rng(0)
    return {"clustered": U.clustered_scene(rng, 500), "sparse": U.sparse_scene(rng, 500)}


def nms_operators(args):
    factors = torch.tensor(R50_FACTORS, device="cuda")
    for scene, (bx, sc, lb) in nms_scenes().items():
        boxes, scores, labels = (torch.from_numpy(a)[None].to("cuda") for a in (bx, sc, lb))
        count = torch.tensor([500], dtype=torch.int32, device="cuda")
        for kind in ("rotate", "circle"):
            circle = kind == "circle"
            kw = dict(nms_type=kind, threshold=4.0 if circle else 0.2, pre_max_size=None if circle else 1000,
                      post_max_size=83 if circle else 500, rescale_factor=None if circle else R50_FACTORS,
                      bottom_center=True, padded=True)
            ours = lambda: bev.bev_nms(boxes, scores, labels, count, **kw)
            if args.once:
                ours()
                torch.cuda.synchronize()
                continue
            theirs = lambda: torch_nms(boxes[0], scores[0], labels[0], factors, kw["threshold"], kw["post_max_size"], circle)
            got = ours()
            keep, out, _, _ = theirs()
            kept = int(got[3][0])
            same = kept == int(keep.sum()) and torch.equal(got[0][0, :kept], out[keep])
            sup = torch.zeros(500, 500, dtype=torch.bool, device="cuda").triu(1)
            o = stats(graph_times_us(ours, 50, args.rounds))
            t = stats(graph_times_us(theirs, 4, args.rounds))
            scan = stats(graph_times_us(lambda: torch_scan(sup, 500), 4, args.rounds))
            print(json.dumps({"op": "bev_nms", "nms_type": kind, "scene": scene, "num": 500, "kept": kept,
                              "torch_formulation_selects_the_same": bool(same), "us": o, "torch_graph_us": t,
                              "torch_scan_graph_us": scan,
                              "speedup_vs_torch_graph": round(t["median"] / o["median"], 1)}), flush=True)


def bevdet_frame(mode, frames=40):
    """Child of --bevdet-ab: BEVDet-R50 forward + get_candidates / get_bboxes (padded) in one captured graph."""
    from bevformer_tensorrt_amd import bevdet as D
    dev = torch.device("cuda")
    model = D.BEVDet(seed=0).to(dev, torch.float16)
    ranks = [r.to(dev) for r in model.view.get_bev_pool_input(*D.synthetic_rig(model.view))]
    image = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).to(dev, torch.float16)
    post = model.get_bboxes if mode == "bboxes" else model.get_candidates
    step = lambda: post(model(image, *ranks), padded=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(frames):
        g.replay()
    b.record()
    b.synchronize()
    print(json.dumps({"model": "bevdet_r50", "postprocess": mode, "frames": frames,
                      "ms_per_frame": round(a.elapsed_time(b) / frames, 4), "rows": int(out[3][0])}), flush=True)


def bevdet_ab(pairs):
    rows = {"candidates": [], "bboxes": []}
    for _ in range(pairs):
        for mode in rows:
            cmd = [sys.executable, os.path.abspath(__file__), "--bevdet-frame", mode]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                raise SystemExit(f"{' '.join(cmd)} failed with {r.returncode}")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rows[mode].append(rec["ms_per_frame"])
            print(json.dumps(rec), flush=True)
    off, on = statistics.median(rows["candidates"]), statistics.median(rows["bboxes"])
    print(json.dumps({"frame_ab": "bevdet_r50", "pairs": pairs, "ms_get_candidates": rows["candidates"],
                      "ms_get_bboxes": rows["bboxes"], "median_candidates": off, "median_bboxes": on,
                      "delta_us": round((on - off) * 1e3, 1), "delta_percent": round((on / off - 1) * 100, 2)}), flush=True)


def eager_us(fn, rounds, iters=20):
    out = []
    for _ in range(2):
        fn()
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / iters)
    return out


def operators(args):
    g = torch.Generator().manual_seed(0)
    rng = torch.tensor(RANGE, device="cuda")
    for dtype in (torch.float16, torch.float32):
        name = str(dtype).split(".")[-1]
        # BEVFormer base: last decoder level, batch 1
        cls = torch.randn(1, 900, 10, generator=g).to("cuda", dtype)
        box = (torch.randn(1, 900, 10, generator=g) * torch.tensor([40.0, 40, 0.5, 0.5, 6, 0.5, 1, 1, 1, 1])).to("cuda", dtype)
        ours = lambda: bev.nms_free_decode(cls, box, 300, RANGE, bottom_center=True, padded=True)
        theirs = lambda: torch_nms_free(cls[0], box[0], 300, rng)

        def trim():
            b, s, l, m = torch_nms_free(cls[0], box[0], 300, rng)
            return b[m], s[m], l[m]
        if args.once:
            ours()
            torch.cuda.synchronize()
        else:
            o, t = stats(graph_times_us(ours, 50, args.rounds)), stats(graph_times_us(theirs, 50, args.rounds))
            e = stats(eager_us(trim, args.rounds))
            te = stats(eager_us(theirs, args.rounds))
            print(json.dumps({"op": "nms_free_decode", "dtype": name, "num_query": 900, "num_classes": 10, "max_num": 300,
                              "us": o, "torch_graph_us": t, "speedup_vs_torch_graph": round(t["median"] / o["median"], 2),
                              "torch_eager_with_mask_index_us": e, "torch_eager_without_mask_index_us": te}), flush=True)
        # BEVDet-R50: the six head maps, channels-last in fp16 (as the model's convolutions emit them), NCHW in fp32
        mk = lambda c, s=1.0, o=0.0: (torch.randn(1, c, 128, 128, generator=g) * s + o).to("cuda", dtype)
        maps = [mk(2), mk(1, 6.0), mk(3, 0.5), mk(2), mk(2), mk(10, 1.0, -5.2)]
        if dtype == torch.float16:
            maps = [m.contiguous(memory_format=torch.channels_last) for m in maps]
        tail = [500, RANGE, [-51.2, -51.2], 8, [0.1, 0.1], 0.1]
        ours = lambda: bev.centerpoint_decode(*maps, *tail, padded=True)
        theirs = lambda: torch_centerpoint(*maps, 500, rng, 0.1, 8, [0.1, 0.1], [-51.2, -51.2])

        def trim():
            b, s, l, m = torch_centerpoint(*maps, 500, rng, 0.1, 8, [0.1, 0.1], [-51.2, -51.2])
            return b[0, m[0]], s[0, m[0]], l[0, m[0]]
        if args.once:
            ours()
            torch.cuda.synchronize()
            continue
        o, t = stats(graph_times_us(ours, 50, args.rounds)), stats(graph_times_us(theirs, 50, args.rounds))
        e = stats(eager_us(trim, args.rounds))
        te = stats(eager_us(theirs, args.rounds))
        print(json.dumps({"op": "centerpoint_decode", "dtype": name, "layout": "channels_last" if dtype == torch.float16 else "nchw",
                          "num_classes": 10, "H": 128, "W": 128, "max_num": 500, "us": o, "torch_graph_us": t,
                          "speedup_vs_torch_graph": round(t["median"] / o["median"], 2),
                          "torch_eager_with_mask_index_us": e, "torch_eager_without_mask_index_us": te}), flush=True)


def frame_ab(models, pairs):
    base = [sys.executable, os.path.join(ROOT, "tools", "model_bench.py")]
    for model in models:
        rows = {"off": [], "on": []}
        for _ in range(pairs):
            for key, extra in (("off", []), ("on", ["--decode"])):
                cmd = base + [model, "--graph", "--no-clone", "--static-image", "--frames", "40"] + extra
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr[-2000:])
                    raise SystemExit(f"{' '.join(cmd)} failed with {r.returncode}")
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                rows[key].append(rec["ms_per_frame"])
                print(json.dumps(dict(rec, decode=bool(extra))), flush=True)
        off, on = statistics.median(rows["off"]), statistics.median(rows["on"])
        print(json.dumps({"frame_ab": model, "pairs": pairs, "ms_decode_off": rows["off"], "ms_decode_on": rows["on"],
                          "median_off": off, "median_on": on, "delta_us": round((on - off) * 1e3, 1),
                          "delta_percent": round((on / off - 1) * 100, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--frame-ab", nargs="+", metavar="MODEL")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--nms", action="store_true")
    ap.add_argument("--bevdet-ab", action="store_true")
    ap.add_argument("--bevdet-frame", choices=["candidates", "bboxes"])
    args = ap.parse_args()
    if args.frame_ab:
        return frame_ab(args.frame_ab, args.pairs)
    if args.bevdet_ab:
        return bevdet_ab(args.pairs)
    assert torch.cuda.is_available(), "decode_time.py needs the GPU"
    if args.bevdet_frame:
        return bevdet_frame(args.bevdet_frame)
    if args.nms:
        return nms_operators(args)
    operators(args)


if __name__ == "__main__":
    main()
