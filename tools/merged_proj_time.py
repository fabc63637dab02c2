#!/usr/bin/env python3
"""The merged projection launches of a BEVFormer-base frame against the per-layer launches they replace, under HIP-graph
replay, old and new alternately, three rounds each (the protocol of tools/tsgemm_time.py --ab): one JSON line per site
with every round's figure, the bytes each route must move and the keep rule (worst new round < best old round).
  tsa.value_proj   six layers x 80 000 x 256 (TSA's key stack)       6 x tile_gemm        -> tsgemm_grouped  (passes here,
                   loses in the frame -- the sampler then reads its planes from HBM -- and is not in the model: design/dense.md)
  dec.value_proj   six layers x 40 000 x 256 (bev_embed)             6 x tsgemm           -> tsgemm_grouped
  tsa.prev_term    six layers x 40 000 x 192, identity each          6 x tile_gemm        -> tile_gemm_dst, N = 1152
  sca.off_weights  one layer, 40 000 x (512 | 256)                   tile_gemm + tsgemm   -> tile_gemm_dst, N = 768
  dec.off_weights  one layer, 900 x (64 | 32), identity each         2 x small_gemm       -> small_gemm_dst, N = 96
`old` runs the kernels the frame's dispatch runs per layer; `new_equals_old` is the bit comparison of the two routes."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevformer_tensorrt_amd as bev  # noqa: E402


def graph_median_us(fn, iters=10, rounds=4):
    """Median HIP-graph replay of `iters` captured calls, microseconds per call."""
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


def sites(g, K=256):
    def rnd(*shape, s=1.0):
        return (torch.randn(*shape, generator=g) * s).half().cuda()

    for name, M, old_fn in (("tsa.value_proj", 80000, bev.tile_gemm), ("dec.value_proj", 40000, bev.tsgemm)):
        x, w, b = rnd(M, K, s=0.5), rnd(6 * 256, K, s=K ** -0.5), rnd(6 * 256)
        ws, bs = [w[i * 256:(i + 1) * 256].contiguous() for i in range(6)], [b[i * 256:(i + 1) * 256].contiguous() for i in range(6)]
        out, outs = torch.empty(6, M, 256, dtype=torch.half, device="cuda"), [torch.empty(M, 256, dtype=torch.half, device="cuda") for _ in range(6)]
        yield (name, lambda: [old_fn(x, ws[i], bs[i], out=outs[i]) for i in range(6)], lambda: bev.tsgemm_grouped(x, w, b, out=out),
               lambda: all(torch.equal(out[i], outs[i]) for i in range(6)),
               6 * (M * K + 256 * K + M * 256) * 2, (M * K + 6 * 256 * K + 6 * M * 256) * 2)
    M = 40000
    x, w = rnd(M, K, s=0.5), rnd(6 * 192, K, s=K ** -0.5)
    ws, res = [w[i * 192:(i + 1) * 192].contiguous() for i in range(6)], [rnd(M, 192) for _ in range(6)]
    outs, new = [torch.empty(M, 192, dtype=torch.half, device="cuda") for _ in range(6)], [torch.empty(M, 192, dtype=torch.half, device="cuda") for _ in range(6)]
    yield ("tsa.prev_term", lambda: [bev.tile_gemm(x, ws[i], None, res[i], out=outs[i]) for i in range(6)],
           lambda: bev.tile_gemm_dst(x, w, None, [192] * 6, res, outs=new), lambda: all(torch.equal(a, b) for a, b in zip(new, outs)),
           6 * (M * K + 192 * K + 2 * M * 192) * 2, (M * K + 6 * 192 * K + 12 * M * 192) * 2)
    x, w, b = rnd(M, K, s=0.5), rnd(768, K, s=K ** -0.5), rnd(768)
    w0, w1, b0, b1 = w[:512].contiguous(), w[512:].contiguous(), b[:512].contiguous(), b[512:].contiguous()
    o0, o1 = torch.empty(M, 512, dtype=torch.half, device="cuda"), torch.empty(M, 256, dtype=torch.half, device="cuda")
    n0, n1 = torch.empty_like(o0), torch.empty_like(o1)
    yield ("sca.off_weights", lambda: (bev.tile_gemm(x, w0, b0, out=o0), bev.tsgemm(x, w1, b1, out=o1)),
           lambda: bev.tile_gemm_dst(x, w, b, [512, 256], outs=[n0, n1]), lambda: torch.equal(n0, o0) and torch.equal(n1, o1),
           (2 * M * K + 768 * K + M * 768) * 2, (M * K + 768 * K + M * 768) * 2)


    M = 900      # the decoder's object queries
    x, w = rnd(M, K, s=0.5), rnd(96, K, s=K ** -0.5)
    wa, wb, ra, rb = w[:64].contiguous(), w[64:].contiguous(), rnd(M, 64), rnd(M, 32)
    oa, ob = torch.empty(M, 64, dtype=torch.half, device="cuda"), torch.empty(M, 32, dtype=torch.half, device="cuda")
    na, nb = torch.empty_like(oa), torch.empty_like(ob)
    yield ("dec.off_weights", lambda: (bev.small_gemm(x, wa, None, ra, out=oa), bev.small_gemm(x, wb, None, rb, out=ob)),
           lambda: bev.small_gemm_dst(x, w, None, [64, 32], [ra, rb], outs=[na, nb]), lambda: torch.equal(na, oa) and torch.equal(nb, ob),
           (2 * M * K + 96 * K + 2 * M * 96) * 2, (M * K + 96 * K + 2 * M * 96) * 2)


def main(rounds=3):
    for name, old, new, equal, bytes_old, bytes_new in sites(torch.Generator().manual_seed(0)):
        old(); new()
        same = bool(equal())
        us = {"old": [], "new": []}
        for _ in range(rounds):
            us["old"].append(round(graph_median_us(old), 2))
            us["new"].append(round(graph_median_us(new), 2))
        print(json.dumps({"site": name, "us_old": us["old"], "us_new": us["new"], "new_equals_old": same, "bytes_old": bytes_old,
                          "bytes_new": bytes_new, "keep": max(us["new"]) < min(us["old"])}), flush=True)


if __name__ == "__main__":
    main()
