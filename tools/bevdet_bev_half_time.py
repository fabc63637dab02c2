#!/usr/bin/env python3
"""BEVDet-R50 with bev_half="torch" against bev_half="hip" (bevdet.py), and the two kernels of csrc/lss_split.hip.

  frame     forward_calibrated under HIP-graph replay, both models in ONE process on one state dict, replayed
            alternately (torch, hip, torch, hip, ...): per alternation the mean of `--replays` replays between two
            events; median and maximum per arm over `--alternations` (>= 5) alternations
  bev_half  the same protocol for the BEV half alone (bev_half_calibrated on fixed image features)
  launches  the kernel nodes of the captured BEV half (everything behind image_features) per arm, read from the captured
            graph itself (hipGraphGetNodes): counted, not estimated
  kernels   per-call HIP-graph replay times of bevops_lss_depth_split and bevops_upsample_bilinear_concat_nhwc at the
            R50 shapes, next to the framework statements they replace

One JSON line per record, appended to profiles/bevdet_bev_half/<step>.jsonl.  Every step is a child process of its own
under `timeout`; the script stops at the first step that fails.

    python tools/bevdet_bev_half_time.py [--alternations 7] [--replays 20] [--out-dir profiles/bevdet_bev_half]
    python tools/bevdet_bev_half_time.py --step frame      # one step, in this process"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("frame", 420), ("bev_half", 420), ("launches", 300), ("kernels", 240))      # (name, seconds)


def _capture(fn, keep_graph=False):
    """fn warmed on a side stream, then captured -> (graph, outputs)."""
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph(keep_graph=True) if keep_graph else torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = fn()
    return graph, outs


def _replay_ms(graph, replays):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / replays


def _models():
    import torch
    from bevformer_tensorrt_amd import bevdet as D
    hip = D.BEVDet(seed=0, bev_half="hip").cuda().half()
    tor = D.BEVDet(seed=0, bev_half="torch").cuda().half()
    tor.load_state_dict(hip.state_dict())
    calib = hip.view.calibration_matrices(*D.synthetic_rig(hip.view)).cuda()
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda().half()
    return {"torch": tor, "hip": hip}, img, calib


def step_frame(a):
    import torch
    models, img, calib = _models()
    graphs = {}
    for arm, m in models.items():
        m.forward_calibrated(img, calib)                 # (eager: dispatch choices, merged operands)
        graphs[arm] = _capture(lambda m=m: m.forward_calibrated(img, calib))[0]
    for g in graphs.values():
        _replay_ms(g, 5)
    ms = {"torch": [], "hip": []}
    for _ in range(max(5, a.alternations)):
        for arm in ("torch", "hip"):
            ms[arm].append(round(_replay_ms(graphs[arm], a.replays), 4))
    rec = {"step": "frame", "workload": "BEVDet-R50 forward_calibrated, HIP-graph replay, fp16", "replays": a.replays,
           "alternations": len(ms["hip"]), "device": torch.cuda.get_device_name(0)}
    for arm in ("torch", "hip"):
        rec[f"ms_{arm}"] = ms[arm]
        rec[f"median_ms_{arm}"] = round(statistics.median(ms[arm]), 4)
        rec[f"max_ms_{arm}"] = max(ms[arm])
    return [rec]


def step_bev_half(a):
    """The BEV half alone (everything behind image_features) on fixed image features, interleaved like `frame`."""
    import torch
    models, img, calib = _models()
    graphs = {}
    for arm, m in models.items():
        m.forward_calibrated(img, calib)
        x = m.image_features(img.flatten(0, 1))
        graphs[arm] = _capture(lambda m=m, x=x: m.bev_half_calibrated(x, calib))[0]
    for g in graphs.values():
        _replay_ms(g, 5)
    ms = {"torch": [], "hip": []}
    for _ in range(max(5, a.alternations)):
        for arm in ("torch", "hip"):
            ms[arm].append(round(_replay_ms(graphs[arm], a.replays), 4))
    rec = {"step": "bev_half", "workload": "BEVDet-R50 bev_half_calibrated on fixed image features, HIP-graph replay, fp16",
           "replays": a.replays, "alternations": len(ms["hip"]), "device": torch.cuda.get_device_name(0)}
    for arm in ("torch", "hip"):
        rec[f"ms_{arm}"] = ms[arm]
        rec[f"median_ms_{arm}"] = round(statistics.median(ms[arm]), 4)
        rec[f"max_ms_{arm}"] = max(ms[arm])
    return [rec]


def _hip_runtime():
    """The HIP runtime this process has loaded (the one torch ships), as a ctypes handle."""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 in this process")


def _kernel_nodes(graph):
    """(kernel nodes, all nodes) of a torch.cuda.CUDAGraph(keep_graph=True) after capture."""
    rt = _hip_runtime()
    raw = ctypes.c_void_p(int(graph.raw_cuda_graph()))
    n = ctypes.c_size_t(0)
    rt.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    rt.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    if rt.hipGraphGetNodes(raw, None, ctypes.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    nodes = (ctypes.c_void_p * n.value)()
    if rt.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    kernels = 0
    for node in nodes:
        kind = ctypes.c_int(-1)
        if rt.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) != 0:
            raise RuntimeError("hipGraphNodeGetType failed")
        kernels += kind.value == 0                       # hipGraphNodeTypeKernel
    return kernels, n.value


def step_launches(a):
    import torch
    models, img, calib = _models()
    recs = []
    for arm, m in models.items():
        m.forward_calibrated(img, calib)
        x = m.image_features(img.flatten(0, 1))
        graph, _ = _capture(lambda m=m, x=x: m.bev_half_calibrated(x, calib), keep_graph=True)
        kernels, nodes = _kernel_nodes(graph)
        graph.instantiate()
        whole, _ = _capture(lambda m=m: m.forward_calibrated(img, calib), keep_graph=True)
        wk, wn = _kernel_nodes(whole)
        recs.append({"step": "launches", "arm": arm, "bev_half_kernel_nodes": kernels, "bev_half_graph_nodes": nodes,
                     "frame_kernel_nodes": wk, "frame_graph_nodes": wn, "device": torch.cuda.get_device_name(0)})
    return recs


def step_kernels(a):
    import torch
    import torch.nn.functional as F
    from bevformer_tensorrt_amd import functions as ops
    from bevformer_tensorrt_amd.functions.linear import graph_time_us
    g = torch.Generator().manual_seed(0)
    dev = torch.cuda.get_device_name(0)
    recs = []
    # depth split at R50: 6 cameras x 16 x 44 pixels, the 128-column rows of the merged depth_net GEMM
    y = torch.randn(6 * 704, 128, generator=g).half().cuda()
    nchw = torch.randn(6, 123, 16, 44, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)

    def torch_split():
        depth = nchw[:, :59].softmax(dim=1)
        feat = nchw[:, 59:123].permute(0, 2, 3, 1)
        return depth.contiguous(), feat.contiguous()
    us = {"hip": [], "torch": []}
    for _ in range(a.rounds):
        us["hip"].append(round(graph_time_us(lambda: ops.lss_depth_split(y, 6, 59, 64, 64, 0, spatial=(16, 44))), 2))
        us["torch"].append(round(graph_time_us(torch_split), 2))
    recs.append({"step": "kernels", "kernel": "bevops_lss_depth_split", "shape": "n 6, hw 704, D 59, C 64, row 128",
                 "bytes_in": y.numel() * 2, "bytes_out": 6 * 704 * (59 + 64) * 2, "us_hip": us["hip"],
                 "us_torch_statements": us["torch"], "device": dev})
    for name, (ca, cb, hb, h) in (("x4 + concat", (128, 512, 16, 64)), ("x2", (0, 512, 64, 128))):
        b = torch.randn(1, cb, hb, hb, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
        av = torch.randn(1, ca, h, h, generator=g).half().cuda().contiguous(memory_format=torch.channels_last) if ca else None

        def torch_up(av=av, b=b, h=h):
            x = F.interpolate(b, size=(h, h), mode="bilinear", align_corners=True)
            if av is not None:
                x = torch.cat([av, x], 1)
            return x.contiguous(memory_format=torch.channels_last)
        us = {"hip": [], "torch": []}
        for _ in range(a.rounds):
            us["hip"].append(round(graph_time_us(lambda: ops.upsample_bilinear_concat_nhwc(av, b, size=(h, h))), 2))
            us["torch"].append(round(graph_time_us(torch_up), 2))
        out_bytes = h * h * (ca + cb) * 2
        recs.append({"step": "kernels", "kernel": "bevops_upsample_bilinear_concat_nhwc", "shape": f"{name}: {hb}x{hb}x{cb} -> "
                     f"{h}x{h}x{ca + cb}", "bytes_out": out_bytes, "bytes_in": (b.numel() + (av.numel() if ca else 0)) * 2,
                     "us_hip": us["hip"], "us_torch_statements": us["torch"],
                     "write_GBps_hip": round(out_bytes / (min(us["hip"]) * 1e-6) / 1e9, 1), "device": dev})
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "bevdet_bev_half"))
    a = ap.parse_args()
    if a.step is None:
        for name, seconds in STEPS:
            cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name,
                   "--alternations", str(a.alternations), "--replays", str(a.replays), "--rounds", str(a.rounds),
                   "--out-dir", a.out_dir]
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                print(f"step {name} ended with status {rc}: stopping", file=sys.stderr)
                return rc
        return 0
    import torch
    with torch.no_grad():
        recs = {"frame": step_frame, "bev_half": step_bev_half, "launches": step_launches, "kernels": step_kernels}[a.step](a)
    torch.cuda.synchronize()
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, a.step + ".jsonl"), "a") as f:
        for r in recs:
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
