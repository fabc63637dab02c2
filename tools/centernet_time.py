#!/usr/bin/env python3
"""CenterNet-R18 (centernet.py): the three transposed convolutions of its neck against the library, and the whole fast
path against the plain fp16 path.

  layers  per layer of CTResNetNeck (256 / 128 / 64 channels) at the layer's input size: `conv_transpose2d_nhwc`
          (csrc/deconv.hip, bias + ReLU in its epilogue) against F.conv_transpose2d on channels-last fp16 tensors +
          bias_act_nhwc_
  model   `CenterNet.forward` on the fast path against the plain path on the same fp16 state dict

Both under HIP-graph replay, both sides in ONE process, replayed alternately (library, hip, library, hip, ...): per
alternation the mean of `--replays` replays between two events; median and maximum per arm over `--alternations` (>= 5)
alternations.  Image shapes: (1, 3, 512, 512) and the reference's default engine shape (32, 3, 672, 672)
(configs/centernet/centernet_resnet18_dcnv2_140e_coco_trt.py: default_shapes).

One JSON line per record, appended to <out-dir>/<step>.jsonl.  Every step is a child process of its own under `timeout`;
the script stops at the first step that fails.

    python tools/centernet_time.py [--alternations 7] [--replays 20] [--out-dir profiles/centernet]
    python tools/centernet_time.py --step layers      # one step, in this process"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("layers", 300), ("model", 420))      # (name, seconds)
SHAPES = ((1, 3, 512, 512), (32, 3, 672, 672))


def _capture(fn):
    """fn warmed on a side stream, then captured -> (graph, its outputs): the package's own routine."""
    from bevformer_tensorrt_amd.graph_runner import capture
    return capture(fn)


def _replay_ms(graph, replays):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / replays


def _alternate(graphs, a):
    """{arm: [ms per replay, one value per alternation]} of the arms' graphs replayed in turn."""
    for g in graphs.values():
        _replay_ms(g, 5)
    ms = {arm: [] for arm in graphs}
    for _ in range(max(5, a.alternations)):
        for arm, g in graphs.items():
            ms[arm].append(round(_replay_ms(g, a.replays), 4))
    return ms


def _summary(rec, ms):
    for arm, v in ms.items():
        rec[f"ms_{arm}"] = v
        rec[f"median_ms_{arm}"] = round(statistics.median(v), 4)
        rec[f"max_ms_{arm}"] = max(v)
    return rec


def step_layers(a):
    import torch
    import torch.nn.functional as F
    from bevformer_tensorrt_amd import functions as ops
    g = torch.Generator().manual_seed(0)
    dev = torch.cuda.get_device_name(0)
    recs = []
    for B, _, H, W in SHAPES:
        for i, c in enumerate((256, 128, 64)):
            h, w = (H // 32) << i, (W // 32) << i
            x = torch.randn(B, c, h, w, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
            wt = (torch.randn(c, c, 4, 4, generator=g) / (4 * c) ** 0.5).half().cuda()
            bias = torch.randn(c, generator=g).half().cuda()

            def library(x=x, wt=wt, bias=bias):
                y = F.conv_transpose2d(x, wt, None, 2, 1)
                if not y.is_contiguous(memory_format=torch.channels_last):
                    y = y.contiguous(memory_format=torch.channels_last)
                return ops.bias_act_nhwc_(y, bias, None, True)

            def hip(x=x, wt=wt, bias=bias):
                return ops.conv_transpose2d_nhwc(x, wt, bias, relu=True)
            err = float((library().float() - hip().float()).abs().max())
            graphs = {"library": _capture(library), "hip": _capture(hip)}
            ms = _alternate({k: v[0] for k, v in graphs.items()}, a)
            out_bytes, in_bytes = B * 4 * h * w * c * 2, B * h * w * c * 2 + 16 * c * c * 2
            rec = {"step": "layers", "layer": f"deconv {c} -> {c}", "input": [B, c, h, w], "image": [B, 3, H, W],
                   "gflop": round(2.0 * B * h * w * 4 * 4 * c * c / 1e9, 3), "bytes_in": in_bytes, "bytes_out": out_bytes,
                   "max_abs_diff_library_vs_hip": err, "replays": a.replays, "device": dev}
            _summary(rec, ms)
            rec["GBps_hip"] = round((in_bytes + out_bytes) / (rec["median_ms_hip"] * 1e-3) / 1e9, 1)
            recs.append(rec)
    return recs


def step_model(a):
    import types
    import torch
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.centernet import CenterNet
    fast = CenterNet(seed=0).cuda().half()
    plain_ops = types.SimpleNamespace(modulated_deformable_conv2d=fn.modulated_deformable_conv2d)
    plain = CenterNet(seed=0, ops=plain_ops).cuda().half()
    plain.load_state_dict(fast.state_dict())
    recs = []
    for shape in SHAPES:
        img = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda().half()
        outs = {"plain": plain(img), "fast": fast(img)}           # (eager: packed and merged operands)
        err = [float((p.float() - f.float()).abs().max()) for p, f in zip(outs["plain"], outs["fast"])]
        del outs
        graphs = {"plain": _capture(lambda: plain(img)), "fast": _capture(lambda: fast(img))}
        ms = _alternate({k: v[0] for k, v in graphs.items()}, a)
        recs.append(_summary({"step": "model", "workload": "CenterNet-R18-DCNv2 forward, HIP-graph replay, fp16",
                              "image": list(shape), "max_abs_diff_plain_vs_fast": err, "replays": a.replays,
                              "device": torch.cuda.get_device_name(0)}, ms))
        del graphs
        torch.cuda.empty_cache()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "centernet"))
    a = ap.parse_args()
    if a.step is None:
        for name, seconds in STEPS:
            cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name,
                   "--alternations", str(a.alternations), "--replays", str(a.replays), "--out-dir", a.out_dir]
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                print(f"step {name} ended with status {rc}: stopping", file=sys.stderr)
                return rc
        return 0
    import torch
    with torch.no_grad():
        recs = {"layers": step_layers, "model": step_model}[a.step](a)
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
