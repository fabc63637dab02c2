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
--once: every decode once, eagerly, no timing (for a `rocprofv3 --kernel-trace --stats` run: launches per call).
--frame-ab: the whole frame with FrameRunner(decode=True) against decode=False as interleaved same-box pairs, each a
fresh `tools/model_bench.py MODEL --graph --no-clone --static-image --frames 40 [--decode]` process."""
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
    args = ap.parse_args()
    if args.frame_ab:
        return frame_ab(args.frame_ab, args.pairs)
    assert torch.cuda.is_available(), "decode_time.py needs the GPU"
    operators(args)


if __name__ == "__main__":
    main()
