#!/usr/bin/env python3
"""The INT8 engine's block-ending sites with the LayerNorm in the int8 GEMM's epilogue (bevops_tsgemm_s8_ln) against
today's sequences, at the base frame's 40 000 rows: median HIP-graph replay, old and new alternately, three rounds in one
process; one JSON line per site with every round's figure and the keep decision of design/dense.md (the worst new round
below the best old round).

  ffn          fc1 F16Q -> fp16, fc2 F16Q + identity, layer_norm   |  fc1 F16Q -> int8 (ReLU), bevops_tsgemm_s8_ln
  output_proj  output_proj F16Q + identity, layer_norm             |  quantize_rows, bevops_tsgemm_s8_ln
  kernel       bevops_tsgemm_s8 (fp16 out) + layer_norm            |  bevops_tsgemm_s8_ln        (int8 operand given, K = 512)

    python tools/int8_ln_time.py [--rows 40000] [--out profiles/int8_ln/per_call.jsonl]
    python tools/int8_ln_time.py --old-only      # today's sequences alone: also runs in a checkout without the new entry,
                                                 # to confirm that the untouched kernels time the same in both builds"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevformer_tensorrt_amd.functions as ops  # noqa: E402
from bevformer_tensorrt_amd import bevformer as B  # noqa: E402
from bevformer_tensorrt_amd.functions import int8_chain as C  # noqa: E402
from bevformer_tensorrt_amd.quantization import MinMaxCalibrator, quantize_dense_layers  # noqa: E402


def graph_median_us(fn, iters=10, rounds=4):
    """Median HIP-graph replay of `iters` captured calls, microseconds per call (the protocol of tools/tsgemm_time.py)."""
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
    ms = []
    for _ in range(rounds + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); g.replay(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return 0.5 * (ms[(len(ms) - 1) // 2] + ms[len(ms) // 2]) * 1e3 / iters


def frozen(module, feed):
    """The nn.Linear layers of `module` as min-max-calibrated, frozen LinearQs (`feed()` runs the calibration batch)."""
    q = quantize_dense_layers(module, MinMaxCalibrator())
    for m in q:
        m.calibrate()
    feed()
    for m in q:
        m.freeze()
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=40000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--old-only", action="store_true")
    a = ap.parse_args()
    M = a.rows
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, 256, generator=g).half().cuda()
    ident = torch.randn(M, 256, generator=g).half().cuda()
    norm = torch.nn.LayerNorm(256).cuda().half()
    sites = []
    with torch.no_grad():
        ffn = B.FFN().cuda().half()
        frozen(ffn, lambda: ffn(x, ops, norm))

        switch = getattr(B, "_INT8_LN_FUSED", {"enabled": False})     # (absent in a checkout from before the entry)

        def ffn_with(on):
            def fn():
                prev = switch["enabled"]
                switch["enabled"] = on
                try:
                    return ffn(x, ops, norm)
                finally:
                    switch["enabled"] = prev
            return fn
        # hidden tensor: 2 bytes per element written and read back (old), 1 byte each way (new)
        sites.append(("ffn", M, 512, ffn_with(False), ffn_with(True)))

        holder = torch.nn.Module()
        holder.output_proj = torch.nn.Linear(256, 256).cuda().half()
        frozen(holder, lambda: holder.output_proj(x))
        lin = holder.output_proj
        sites.append(("output_proj", M, 256, lambda: B._dense_norm(ops, lin, x, ident, norm),
                      lambda: lin.forward_norm_from_q(ops.quantize_rows(x, lin.scale_in), ident, norm)))

        fc2 = ffn.fc2
        h_q = C.linear_int8_chain(x, ffn.fc1.scale_in, ffn.fc1.weight_q, ffn.fc1.scale_w, ffn.fc1.bias_f32, None, 1.0, True,
                                  torch.int8, fc2.scale_in)

        def pair():
            prev = C._TS_S8["enabled"]
            C._TS_S8["enabled"] = True
            try:
                y = C.linear_int8_chain(h_q, fc2.scale_in, fc2.weight_q, fc2.scale_w, fc2.bias_f32, ident, 1.0, False,
                                        torch.float16)
            finally:
                C._TS_S8["enabled"] = prev
            return ops.layer_norm(y, norm.weight, norm.bias, norm.eps)
        sites.append(("kernel", M, 512, pair, lambda: fc2.forward_norm_from_q(h_q, ident, norm)))

        lines = []
        for name, rows, K, old, new in sites:
            us = {"old": [], "new": []}
            for _ in range(a.rounds):
                us["old"].append(round(graph_median_us(old), 2))
                if not a.old_only:
                    us["new"].append(round(graph_median_us(new), 2))
            rec = {"site": name, "M": rows, "N": 256, "K": K, "us_old": us["old"], "device": torch.cuda.get_device_name(0)}
            if not a.old_only:
                d = (old().float() - new().float()).abs()
                rec.update(us_new=us["new"], keep=max(us["new"]) < min(us["old"]), max_abs_diff=round(d.max().item(), 5),
                           mean_abs_diff=round(d.mean().item(), 6))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
