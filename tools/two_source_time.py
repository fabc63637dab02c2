#!/usr/bin/env python3
"""The tail of the first bottleneck of every ResNet stage of a BEVFormer-base frame (6 cameras, fp16): the two launches the
frame ran so far -- the downsample convolution, then conv3 with the identity in its epilogue, each on the kernel the
frame's dispatch picks -- against the one two-source GEMM (bevops_gemm2_f16), under HIP-graph replay, old and new
alternately, three rounds (the protocol of tools/merged_proj_time.py).  One JSON line per stage with every round's
figure, the bytes each route must move, the difference of the two results and the keep rule (worst new round below the
best old round).  usage: two_source_time.py [--rounds 3] [--iters 10]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevformer_tensorrt_amd.functions as ops  # noqa: E402
from bevformer_tensorrt_amd import bevformer as B  # noqa: E402

# stage, input channels, planes, stride, input H x W of the block (928 x 1600 images: 232 x 400 behind the stem)
STAGES = [(1, 64, 64, 1, 232, 400), (2, 256, 128, 2, 232, 400), (3, 512, 256, 2, 116, 200), (4, 1024, 512, 2, 58, 100)]
CAMS = 6


def graph_of(fn, iters):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g, iters, reps=5):
    """Median of `reps` timed replays, microseconds per call."""
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); g.replay(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2] * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    torch.manual_seed(0)
    for stage, cin, planes, stride, H, W in STAGES:
        blk = B.Bottleneck(cin, planes, stride, False, ops, True).cuda().half().eval()
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        M, N = CAMS * Ho * Wo, 4 * planes
        x = (torch.randn(CAMS, cin, H, W, device="cuda") * 0.5).half().contiguous(memory_format=torch.channels_last)
        h = (torch.randn(CAMS, planes, Ho, Wo, device="cuda") * 0.5).half().contiguous(memory_format=torch.channels_last)
        w, b = B._stacked_pair(blk)
        out = torch.empty(M, N, dtype=torch.half, device="cuda")

        def old():
            with torch.no_grad():
                return B._conv1x1_nhwc(ops, h, blk.conv3, True, residual=B._conv1x1_nhwc(ops, x, blk.downsample, False))

        def new():
            return ops.gemm2(B._rows(h), x, w, b, stride, True, out=out)
        d = (B._rows(old()).float() - new().float()).abs()
        g_old, g_new = graph_of(old, args.iters), graph_of(new, args.iters)
        t_old, t_new = [], []
        for _ in range(args.rounds):
            t_old.append(round(replay_us(g_old, args.iters), 1))
            t_new.append(round(replay_us(g_new, args.iters), 1))
        xs = CAMS * Ho * Wo * cin
        common = (M * planes + xs + N * (planes + cin) + M * N) * 2
        print(json.dumps(dict(stage=stage, M=M, N=N, K1=planes, K2=cin, stride=stride, old_us=t_old, new_us=t_new,
                              old_MB=round((common + 2 * M * N * 2) / 1e6, 1), new_MB=round(common / 1e6, 1),
                              new_TBps=round(common / min(t_new) / 1e6, 2), max_diff=d.max().item(), mean_diff=d.mean().item(),
                              keep=max(t_new) < min(t_old), saved_us=round(min(t_old) - max(t_new), 1))), flush=True)


if __name__ == "__main__":
    main()
