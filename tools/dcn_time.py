#!/usr/bin/env python3
"""HIP-event timing of the BEVFormer-base DCN call shapes per kernel variant.

  dcn_time.py [VARIANT ...]                  the plugin entry, eager calls (default variants 0 2 1)
  dcn_time.py --ab PARENT,NEW[,NEW2 ...] [--rounds 3] [--out FILE.jsonl]
      the channels-last entry (raw offset-convolution operand, bias, ReLU) as the frame launches it: one captured HIP
      graph of CALLS calls per variant, the variants' graphs replayed in turn within a round; stage 3, stage 4 and one
      camera of stage 3.  One JSON row per (shape, round, variant): median and minimum microseconds per call."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bevformer_tensorrt_amd as bev  # noqa: E402
from bevformer_tensorrt_amd.utils import load_library  # noqa: E402
from msda_sweep import time_call  # noqa: E402

CALLS, REPLAYS = 10, 30


def eager(lib, variants):
    g = torch.Generator().manual_seed(0)
    for (C, H, W) in ((256, 58, 100), (512, 29, 50)):
        x = torch.randn(6, C, H, W, generator=g).half().cuda()
        off = torch.randn(6, 18, H, W, generator=g).half().cuda()
        mask = torch.rand(6, 9, H, W, generator=g).half().cuda()
        w = (torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5).half().cuda()
        b = torch.randn(C, generator=g).half().cuda()
        for v in variants:
            lib.bevops_mdconv_set_variant(v)
            med, mn = time_call(lambda: bev.modulated_deformable_conv2d(x, off, mask, w, b, 1, 1, 1, 1, 1))
            lib.bevops_mdconv_set_variant(0)
            fl = 2.0 * 6 * H * W * C * C * 9
            print(json.dumps(dict(shape=[6, C, H, W], variant=v, us_med=round(med, 1), us_min=round(mn, 1),
                                  TFLOPs=round(fl / med / 1e6, 1))), flush=True)


def ab(lib, variants, rounds, out):
    g = torch.Generator().manual_seed(0)
    cl = lambda t: t.half().cuda().contiguous(memory_format=torch.channels_last)
    rows = []
    for name, (B, C, H, W) in (("stage3", (6, 256, 58, 100)), ("stage4", (6, 512, 29, 50)), ("stage3_one_camera", (1, 256, 58, 100))):
        x = cl(torch.randn(B, C, H, W, generator=g))
        om = torch.randn(B, 32, H, W, generator=g)
        om[:, 18:27] *= 1.5
        om = cl(om)
        w = (torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5).half().cuda()
        b = torch.randn(C, generator=g).half().cuda()
        call = lambda: bev.modulated_deformable_conv2d_nhwc(x, None, None, w, b, 1, 1, 1, 1, 1, relu=True, offset_mask_nhwc=om)
        graphs, outs = {}, {}
        for v in variants:
            lib.bevops_mdconv_set_variant(v)
            call()
            torch.cuda.synchronize()
            graphs[v] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[v]):
                for _ in range(CALLS):
                    outs[v] = call()
            lib.bevops_mdconv_set_variant(0)
            graphs[v].replay()
        torch.cuda.synchronize()
        same = all(torch.equal(outs[v], outs[variants[0]]) for v in variants)
        for rnd in range(rounds):
            ts = {v: [] for v in variants}
            for _ in range(REPLAYS):
                for v in variants:
                    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); graphs[v].replay(); e.record()
                    e.synchronize()
                    ts[v].append(a.elapsed_time(e) * 1e3 / CALLS)
            for v in variants:
                t = sorted(ts[v])
                rows.append(dict(shape=name, dims=[B, C, H, W], round=rnd, variant=v, us_med=round(t[len(t) // 2], 2),
                                 us_min=round(t[0], 2), bit_equal=same))
                print(json.dumps(rows[-1]), flush=True)
    if out:
        with open(out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("variants", nargs="*", type=int)
    ap.add_argument("--ab", help="comma-separated variants, the parent skeleton first (10,20,0)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    handle = load_library()
    if a.ab:
        ab(handle, [int(v) for v in a.ab.split(",")], a.rounds, a.out)
    else:
        eager(handle, a.variants or [0, 2, 1])
