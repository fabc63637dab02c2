#!/usr/bin/env python3
"""tsgemm vs the library GEMM paths on the dense-layer shapes of BEVFormer-base (interleaved, HIP events)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bevformer_tensorrt_amd as bev  # noqa: E402
from bevformer_tensorrt_amd import bevformer as B  # noqa: E402
from msda_sweep import time_call  # noqa: E402

SHAPES = [("s3.conv1", 34800, 256, 1024, False, True), ("s3.conv3", 34800, 1024, 256, True, True),
          ("s2.conv3", 139200, 512, 128, True, True), ("s1.conv3", 556800, 256, 64, True, True),
          ("s4.conv1", 8700, 512, 2048, False, True), ("s4.conv3", 8700, 2048, 512, True, True),
          ("s3.down", 34800, 1024, 512, False, False), ("fpn.lat2", 34800, 256, 1024, False, False),
          ("sca.value_proj", 184950, 256, 256, False, False), ("tsa.value_proj", 80000, 256, 256, False, False),
          ("enc.output_proj", 40000, 256, 256, True, False), ("ffn.fc1", 40000, 512, 256, False, True),
          ("ffn.fc2", 40000, 256, 512, True, False)]



def graph_median_us(fn, iters=10, rounds=4):
    """Median HIP-graph replay of `iters` captured calls, microseconds per call (bench.py's graph_us protocol)."""
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


def ab_old_new(rounds=3):
    """--ab: the original kernel (bevops_tsgemm_set_variant(1)) against the weight-stationary one (0) on every K <= 256
    dense layer of a base frame, alternately, under graph replay; one JSON line per layer with every round's figure (the
    spread between rounds of one variant is that layer's noise), the bytes the call must move and the TB/s of the
    medians."""
    from bevformer_tensorrt_amd.utils import lib as L
    handle = L.load_library()
    levels = [[116, 200], [58, 100], [29, 50], [15, 25]]
    nk = sum(h * w for h, w in levels)
    g = torch.Generator().manual_seed(0)
    gam, bet = torch.ones(256).half().cuda(), torch.zeros(256).half().cuda()
    layers = [  # name, kind, M, N, K, residual, relu
        ("sca.value_proj(packed)", "packed", 6 * nk, 256, 256, False, False),
        ("sca.value_proj", "gemm", 6 * nk, 256, 256, False, False),
        ("enc.output_proj+ln", "ln", 40000, 256, 256, True, False),
        ("tsa.value_proj", "gemm", 80000, 256, 256, False, False),
        ("dec.value_proj", "gemm", 40000, 256, 256, False, False),
        ("ffn.fc1", "gemm", 40000, 512, 256, False, True),
        ("s3.conv3", "gemm", 34800, 1024, 256, True, True),
        ("s2.conv3", "gemm", 139200, 512, 128, True, True),
        ("s1.conv3", "gemm", 556800, 256, 64, True, True),
    ]
    for name, kind, M, N, K, has_res, relu in layers:
        x = (torch.randn(M, K, generator=g) * 0.5).half().cuda()
        w = (torch.randn(N, K, generator=g) / K ** 0.5).half().cuda()
        b = torch.randn(N, generator=g).half().cuda()
        r = torch.randn(M, N, generator=g).half().cuda() if has_res else None
        byt = (M * K + N * K + M * N * (2 if has_res else 1)) * 2
        if kind == "packed":
            sh = torch.tensor(levels, dtype=torch.int32)
            nbytes = handle.bevops_value_proj_packed_size(sh.data_ptr(), 6, nk, 8, 32, 4, 40000, 8)
            planes = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            byt = (M * K + N * K) * 2 + nbytes - ((6 * 40000 * 8 + 255) // 256) * 256   # rows in, padded planes out
            fn = lambda: L.check(handle.bevops_value_proj_packed(
                x.data_ptr(), w.data_ptr(), b.data_ptr(), sh.data_ptr(), planes.data_ptr(), nbytes, 6, nk, 8, 32, 4, 40000, 8,
                L.current_stream_ptr(x.device)), "bevops_value_proj_packed")
        elif kind == "ln":
            fn = lambda: bev.tsgemm_ln(x, w, b, r, gam, bet, 1e-5)
        else:
            out = torch.empty(M, N, dtype=torch.half, device="cuda")
            fn = lambda: bev.tsgemm(x, w, b, r, relu, out=out)
        us = {"old": [], "new": []}
        for _ in range(rounds):
            for tag, variant in (("old", 1), ("new", 0)):
                prev = handle.bevops_tsgemm_set_variant(variant)
                try:
                    us[tag].append(round(graph_median_us(fn), 2))
                finally:
                    handle.bevops_tsgemm_set_variant(prev)
        med = {t: sorted(v)[len(v) // 2] for t, v in us.items()}
        print(json.dumps({"layer": name, "M": M, "N": N, "K": K, "us_old": us["old"], "us_new": us["new"], "bytes": byt,
                          "TBs_old": round(byt / med["old"] / 1e6, 2), "TBs_new": round(byt / med["new"] / 1e6, 2),
                          "keep": max(us["new"]) < min(us["old"])}), flush=True)


def once_old_new():
    """--once: one launch of the original and one of the weight-stationary kernel on value_proj (through
    bevops_value_proj_packed), FFN fc1 and stage-3 conv3 -- the process to put under a counter run of its own
    (rocprofv3 --pmc FETCH_SIZE WRITE_SIZE -- python tools/tsgemm_time.py --once)."""
    from bevformer_tensorrt_amd.utils import lib as L
    handle = L.load_library()
    levels = [[116, 200], [58, 100], [29, 50], [15, 25]]
    nk = sum(h * w for h, w in levels)
    g = torch.Generator().manual_seed(0)
    sh = torch.tensor(levels, dtype=torch.int32)
    nbytes = handle.bevops_value_proj_packed_size(sh.data_ptr(), 6, nk, 8, 32, 4, 40000, 8)
    planes = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for M, N, K, has_res in ((6 * nk, 256, 256, False), (40000, 512, 256, False), (34800, 1024, 256, True)):
        x = (torch.randn(M, K, generator=g) * 0.5).half().cuda()
        w = (torch.randn(N, K, generator=g) / K ** 0.5).half().cuda()
        b = torch.randn(N, generator=g).half().cuda()
        r = torch.randn(M, N, generator=g).half().cuda() if has_res else None
        for variant in (1, 0):
            prev = handle.bevops_tsgemm_set_variant(variant)
            try:
                if N == 256:
                    L.check(handle.bevops_value_proj_packed(x.data_ptr(), w.data_ptr(), b.data_ptr(), sh.data_ptr(), planes.data_ptr(),
                                                            nbytes, 6, nk, 8, 32, 4, 40000, 8, L.current_stream_ptr(x.device)), "vp")
                else:
                    bev.tsgemm(x, w, b, r, has_res)
                torch.cuda.synchronize()
            finally:
                handle.bevops_tsgemm_set_variant(prev)


if "--ab" in sys.argv:
    ab_old_new()
    sys.exit(0)
if "--once" in sys.argv:
    once_old_new()
    sys.exit(0)

B.use_tuned_gemms()
for name, M, N, K, has_res, relu in SHAPES:
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, K, generator=g).half().cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).half().cuda()
    b = torch.randn(N, generator=g).half().cuda()
    r = torch.randn(M, N, generator=g).half().cuda() if has_res else None
    wt = w.t()
    if has_res:
        lib = lambda: bev.linear_bias_act(x, w, b, r, relu)
    elif relu:
        lib = lambda: torch._addmm_activation(b, x, wt)
    else:
        lib = lambda: torch.addmm(b, x, wt)
    ours = lambda: bev.tsgemm(x, w, b, r, relu)
    res = {"lib": [], "ts": []}
    for _ in range(3):
        res["lib"].append(round(time_call(lib, iters=20, warm=5)[0], 1))
        res["ts"].append(round(time_call(ours, iters=20, warm=5)[0], 1))
    byt = (M * K + N * K + M * N * (2 if has_res else 1)) * 2
    ts = sorted(res["ts"])[1]
    print(json.dumps({"layer": name, "M": M, "N": N, "K": K, "us_lib": sorted(res["lib"])[1], "us_tsgemm": ts,
                      "GBs_tsgemm": round(byt / ts / 1e3, 1), "TFLOPs_tsgemm": round(2.0 * M * N * K / ts / 1e6, 1)}), flush=True)
