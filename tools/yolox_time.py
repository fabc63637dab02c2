#!/usr/bin/env python3
"""YOLOX-x (yolox.py): every distinct convolution shape of its fast path against the library, and the whole fast path
against the plain fp16 path.

  layers  every distinct (Cin, Cout, k, stride, map, activation, identity) of one YOLOX-x forward, as the fast path
          launches it (padded widths, stacked / block-diagonal head operands): `conv_slice_taps` (csrc/conv_slice.hip,
          bias + SiLU + identity in its epilogue) against F.conv2d on channels-last fp16 tensors + a SiLU pass
          (x * sigmoid(x)) + the identity add.  Dense operands on both sides (pitch == channels).  Reports the achieved
          fraction of the fp16 matrix peak (2 516.8 TFLOP/s, the data sheet's dense figure) per layer.
  model   `YOLOX.forward` on the fast path against the plain path on the same fp16 state dict

Both under HIP-graph replay, both sides in ONE process, replayed alternately (library, hip, library, hip, ...): per
alternation the mean of `--replays` replays between two events; median and maximum per arm over `--alternations` (>= 5)
alternations.  Image shapes: (1, 3, 640, 640) and the reference's engine shape (32, 3, 640, 640)
(configs/yolox/yolox_x_8x8_300e_coco_trt.py).

One JSON line per record, appended to <out-dir>/<step>.jsonl.  Every step is a child process of its own under `timeout`;
the script stops at the first step that fails.

    python tools/yolox_time.py [--alternations 7] [--replays 20] [--out-dir profiles/yolox]
    python tools/yolox_time.py --step layers      # one step, in this process"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("layers", 540), ("model", 420))      # (name, seconds)
SHAPES = ((1, 3, 640, 640), (32, 3, 640, 640))
PEAK_FP16_TFLOPS = 2516.8


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


def _alternate(graphs, alternations, replays):
    """{arm: [ms per replay, one value per alternation]} of the arms' graphs replayed in turn."""
    for g in graphs.values():
        _replay_ms(g, 3)
    ms = {arm: [] for arm in graphs}
    for _ in range(max(5, alternations)):
        for arm, g in graphs.items():
            ms[arm].append(round(_replay_ms(g, replays), 4))
    return ms


def _summary(rec, ms):
    for arm, v in ms.items():
        rec[f"ms_{arm}"] = v
        rec[f"median_ms_{arm}"] = round(statistics.median(v), 4)
        rec[f"max_ms_{arm}"] = max(v)
    return rec


def _layer_list(model, shape):
    """The distinct convolution launches of one fast forward at `shape`, in first-use order, with their counts:
    {(Cin, Cout, k, stride, H, W, act, identity): count}; traced on a one-image batch (the shapes do not depend on B)."""
    import types
    import torch
    import bevformer_tensorrt_amd.functions as fn
    seen = {}

    def probe(x, w, b=None, act="silu", residual=None, stride=1, out=None):
        key = (x.shape[1], w.shape[0], w.shape[1], stride, x.shape[2], x.shape[3], act, residual is not None)
        seen[key] = seen.get(key, 0) + 1
        return fn.conv_slice_taps(x, w, b, act, residual, stride, out)

    ops = types.SimpleNamespace(conv_slice_taps=probe, focus_nhwc=fn.focus_nhwc, spp_maxpool_nhwc=fn.spp_maxpool_nhwc,
                                upsample_nearest2x_nhwc=fn.upsample_nearest2x_nhwc)
    saved, model.ops = model.ops, ops
    try:
        model(torch.zeros((1,) + tuple(shape[1:]), device="cuda", dtype=torch.float16))
    finally:
        model.ops = saved
    return seen


def step_layers(a):
    import torch
    import torch.nn.functional as F
    from bevformer_tensorrt_amd import functions as ops
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_X
    g = torch.Generator().manual_seed(0)
    dev = torch.cuda.get_device_name(0)
    model = YOLOX(YOLOX_X, seed=0).cuda().half()
    recs = []
    for shape in SHAPES:
        B = shape[0]
        replays = a.replays if B == 1 else max(3, a.replays // 4)
        for (cin, cout, k, stride, h, w, act, idt), count in _layer_list(model, shape).items():
            x = torch.randn(B, cin, h, w, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
            wt = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).half().cuda()
            taps = wt.permute(0, 2, 3, 1).contiguous()
            bias = torch.randn(cout, generator=g).half().cuda()
            ho, wo = (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1
            res = torch.randn(B, cout, ho, wo, generator=g).half().cuda().contiguous(memory_format=torch.channels_last) \
                if idt else None

            def library(x=x, wt=wt, bias=bias, res=res, act=act, stride=stride, k=k):
                y = F.conv2d(x, wt, bias, stride, k // 2)
                if act == "silu":
                    y = y * torch.sigmoid(y)
                return y if res is None else y + res

            def hip(x=x, taps=taps, bias=bias, res=res, act=act, stride=stride):
                return ops.conv_slice_taps(x, taps, bias, act, res, stride)
            err = float((library().float() - hip().float()).abs().max())
            graphs = {"library": _capture(library), "hip": _capture(hip)}
            ms = _alternate({n: v[0] for n, v in graphs.items()}, a.alternations, replays)
            gflop = 2.0 * B * ho * wo * k * k * cin * cout / 1e9
            rec = {"step": "layers", "layer": f"conv {cin} -> {cout} {k}x{k} / {stride} {act}{' + identity' if idt else ''}",
                   "input": [B, cin, h, w], "image": list(shape), "launches_per_forward": count, "gflop": round(gflop, 3),
                   "max_abs_diff_library_vs_hip": err, "replays": replays, "device": dev}
            _summary(rec, ms)
            rec["tflops_hip"] = round(gflop / rec["median_ms_hip"], 1)
            rec["fraction_of_fp16_peak_hip"] = round(gflop / rec["median_ms_hip"] / PEAK_FP16_TFLOPS, 4)
            rec["hip_over_library"] = round(rec["median_ms_hip"] / rec["median_ms_library"], 3)
            recs.append(rec)
            del graphs, x, res
        torch.cuda.empty_cache()
    return recs


def step_model(a):
    import types
    import torch
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_X
    fast = YOLOX(YOLOX_X, seed=0).cuda().half()
    plain = YOLOX(YOLOX_X, seed=0, ops=types.SimpleNamespace()).cuda().half()
    plain.load_state_dict(fast.state_dict())
    recs = []
    for shape in SHAPES:
        replays = a.replays if shape[0] == 1 else max(3, a.replays // 4)
        img = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda().half()
        outs = {"plain": plain(img), "fast": fast(img)}           # (eager: merged and padded operands)
        err = [float((p.float() - f.float()).abs().max()) for p, f in zip(outs["plain"], outs["fast"])]
        del outs
        graphs = {"plain": _capture(lambda: plain(img)), "fast": _capture(lambda: fast(img))}
        ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, replays)
        recs.append(_summary({"step": "model", "workload": "YOLOX-x forward, HIP-graph replay, fp16",
                              "image": list(shape), "max_abs_diff_plain_vs_fast": err, "replays": replays,
                              "device": torch.cuda.get_device_name(0)}, ms))
        del graphs
        torch.cuda.empty_cache()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "yolox"))
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
