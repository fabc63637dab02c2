#!/usr/bin/env python3
"""qkv and inverse (csrc/qkv.hip, csrc/inverse.hip) timed under HIP-graph replay against the framework's own ops on the
same tensors: torch.nn.functional.scaled_dot_product_attention and torch.linalg.inv_ex (inv_ex: torch.linalg.inv checks
its result on the host, which a captured graph cannot hold).  Per shape: the median and the max over >= 5 rounds of
one replay of `iters` calls each, the FLOPs 4 B Lq Lkv E and the fraction of the fp16 / fp32 matrix peak
(MI355X: 2.5 PF dense fp16, 157.3 TF fp32).  One JSON line per (op, dtype, shape).
    python tools/qkv_time.py [--rounds 7] [--once]
--once: every call once, eagerly, no timing (for a `rocprofv3 --kernel-trace --stats` run: launches per call)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevformer_tensorrt_amd as bev  # noqa: E402

QKV_SHAPES = [(64, 960, 960, 32), (8, 900, 900, 32), (8, 900, 2500, 32), (2, 64, 40000, 32), (16, 1024, 1024, 64),
              (8, 512, 777, 128), (3, 1, 1, 16), (5, 31, 33, 48)]
INV_SHAPES = [(2048, 32), (6, 3), (2048, 3), (512, 4), (512, 16)]
PEAK_TFLOPS = {torch.float16: 2500.0, torch.float32: 157.3}


def graph_times_us(fn, iters, rounds):
    """Per-call microseconds of `iters` captured calls, one number per replay round."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.float16, torch.float32):
        for B, Lq, Lkv, E in QKV_SHAPES:
            q = torch.randn(B, Lq, E, generator=g).to("cuda", dtype)
            k = torch.randn(B, Lkv, E, generator=g).to("cuda", dtype)
            v = torch.randn(B, Lkv, E, generator=g).to("cuda", dtype)
            if args.once:
                bev.qkv(q, k, v)
                torch.cuda.synchronize()
                continue
            flop = 4.0 * B * Lq * Lkv * E
            iters = max(2, min(50, int(2e10 / flop / (16 if dtype == torch.float32 else 1)) or 2))
            ours = stats(graph_times_us(lambda: bev.qkv(q, k, v), iters, args.rounds))
            sdpa = stats(graph_times_us(lambda: F.scaled_dot_product_attention(q, k, v), iters, args.rounds))
            rec = {"op": "qkv", "dtype": str(dtype).split(".")[-1], "B": B, "Lq": Lq, "Lkv": Lkv, "E": E,
                   "flop": flop, "iters": iters, "us": ours, "sdpa_us": sdpa,
                   "tflops": round(flop / ours["median"] / 1e6, 2),
                   "frac_peak": round(flop / ours["median"] / 1e6 / PEAK_TFLOPS[dtype], 4),
                   "speedup_vs_sdpa": round(sdpa["median"] / ours["median"], 3)}
            print(json.dumps(rec), flush=True)
    for batch, n in INV_SHAPES:
        a = torch.randn(batch, n, n, generator=g).cuda() + n * torch.eye(n, device="cuda")
        if args.once:
            bev.inverse(a)
            torch.cuda.synchronize()
            continue
        ours = stats(graph_times_us(lambda: bev.inverse(a), 20, args.rounds))
        ref = stats(graph_times_us(lambda: torch.linalg.inv_ex(a), 20, args.rounds))
        print(json.dumps({"op": "inverse", "dtype": "float32", "batch": batch, "n": n, "us": ours,
                          "torch_linalg_inv_ex_us": ref, "speedup": round(ref["median"] / ours["median"], 3)}),
              flush=True)


if __name__ == "__main__":
    main()
