#!/usr/bin/env python3
"""INT8 CenterNet (centernet_int8.py) against the fp16 fast path (centernet.py): the two new operators per distinct
layer shape, and the whole forward in both neck modes.

  layers  every distinct deconvolution (256 / 128 / 64 channels at 1/32, 1/16, 1/8 of the image) and every distinct
          BasicBlock conv2 (3x3 + identity + ReLU at 64 / 128 / 256 / 512 channels): `conv_transpose2d_q_nhwc`
          (csrc/deconv_s8.hip) against `conv_transpose2d_nhwc` (csrc/deconv.hip), and `conv_slice_q_taps(res_first=True)`
          (csrc/conv_slice_s8.hip) against the fp16 fast path's choice for that layer (`conv3x3_auto` under the rule
          dispatch).
  model   `Int8CenterNet.forward` with neck="int8" and neck="fp16" against `CenterNet.forward` (fast path) on the same
          weights; calibrated on one random frame with the device min-max calibrator (the scales do not change the time).

All under HIP-graph replay, all arms in ONE process, replayed alternately (fp16, int8, fp16, int8, ...): per alternation
the mean of `--replays` replays between two events; median and maximum per arm over `--alternations` (>= 5)
alternations.  Image shapes: (1, 3, 512, 512) and the reference's engine shape (32, 3, 672, 672).

One JSON line per record, appended to <out-dir>/<step>.jsonl.  Every step is a child process of its own under `timeout`;
the script stops at the first step that fails.

    python tools/centernet_int8_time.py [--alternations 7] [--replays 20] [--out-dir profiles/centernet_int8]
    python tools/centernet_int8_time.py --step layers      # one step, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from yolox_time import _alternate, _capture, _summary   # noqa: E402

SHAPES = ((1, 3, 512, 512), (32, 3, 672, 672))
STEPS = (("layers", 420), ("model", 420))      # (name, seconds)
DECONVS = ((256, 32), (128, 16), (64, 8))      # (channels, the image's size over the input map's)
CONV2S = ((64, 4, 4), (128, 8, 4), (256, 16, 4), (512, 32, 4))      # (channels, divisor, launches per forward)


def _q(t, s):
    import torch
    return torch.clamp(torch.round(t.float() / s), -127, 127).to(torch.int8)


def step_layers(a):
    import torch
    from bevformer_tensorrt_amd import functions as ops
    from bevformer_tensorrt_amd.functions import dispatch
    g = torch.Generator().manual_seed(0)
    dev = torch.cuda.get_device_name(0)
    nhwc = lambda t: t.contiguous(memory_format=torch.channels_last)    # noqa: E731
    sx, sr, so = 5.0 / 127, 5.0 / 127, 12.0 / 127     # unit-normal tensors clip beyond 5 sigma, the outputs beyond 12
    recs = []
    for shape in SHAPES:
        B = shape[0]
        replays = a.replays if B == 1 else max(3, a.replays // 4)
        for c, div in DECONVS:
            h, w = shape[2] // div, shape[3] // div
            x = nhwc(torch.randn(B, c, h, w, generator=g).half().cuda())
            wt = (torch.randn(c, c, 4, 4, generator=g) / (4 * c) ** 0.5).half().cuda()
            bias = torch.randn(c, generator=g).half().cuda()
            x_q = nhwc(_q(x, sx))
            wq, ws, b32 = ops.quantize_deconv_weight(wt, bias)

            def fp16(x=x, wt=wt, bias=bias):
                return ops.conv_transpose2d_nhwc(x, wt, bias, relu=True)

            def int8(x_q=x_q, wq=wq, ws=ws, b32=b32):
                return ops.conv_transpose2d_q_nhwc(x_q, sx, wq, ws, b32, True, so)
            err = float((fp16().float() - int8().float() * so).abs().max())
            graphs = {"fp16": _capture(fp16), "int8": _capture(int8)}
            ms = _alternate({n: v[0] for n, v in graphs.items()}, a.alternations, replays)
            gflop = 2.0 * B * h * w * 16 * c * c / 1e9
            rec = {"step": "layers", "layer": f"deconv {c} -> {c} 4x4 / 2 relu", "input": [B, c, h, w], "image": list(shape),
                   "launches_per_forward": 1, "gflop": round(gflop, 3), "blocks_int8": 4 * ((c + 127) // 128 if c > 64 else 1)
                   * ((B * h * w + 127) // 128), "max_abs_diff_fp16_vs_int8": err, "replays": replays, "device": dev}
            _summary(rec, ms)
            rec["int8_over_fp16"] = round(rec["median_ms_int8"] / rec["median_ms_fp16"], 3)
            recs.append(rec)
            del graphs, x, x_q
        for c, div, count in CONV2S:
            h, w = shape[2] // div, shape[3] // div
            x = nhwc(torch.randn(B, c, h, w, generator=g).half().cuda())
            res = nhwc(torch.randn(B, c, h, w, generator=g).half().cuda())
            wt = (torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5).half().cuda()
            bias = torch.randn(c, generator=g).half().cuda()
            x_q, r_q = nhwc(_q(x, sx)), nhwc(_q(res, sr))
            wq, ws, b32 = ops.quantize_weight_taps(wt, bias)

            def fp16(x=x, wt=wt, bias=bias, res=res):
                with dispatch.using(rule=True):
                    return ops.conv3x3_auto(x, wt, bias, True, res, 1)

            def int8(x_q=x_q, wq=wq, ws=ws, b32=b32, r_q=r_q):
                return ops.conv_slice_q_taps(x_q, sx, wq, ws, b32, "relu", r_q, sr, 1, None, so, torch.int8, res_first=True)
            err = float((fp16().float() - int8().float() * so).abs().max())
            graphs = {"fp16": _capture(fp16), "int8": _capture(int8)}
            ms = _alternate({n: v[0] for n, v in graphs.items()}, a.alternations, replays)
            gflop = 2.0 * B * h * w * 9 * c * c / 1e9
            rec = {"step": "layers", "layer": f"conv2 {c} -> {c} 3x3 + identity relu", "input": [B, c, h, w],
                   "image": list(shape), "launches_per_forward": count, "gflop": round(gflop, 3),
                   "max_abs_diff_fp16_vs_int8": err, "replays": replays, "device": dev}
            _summary(rec, ms)
            rec["int8_over_fp16"] = round(rec["median_ms_int8"] / rec["median_ms_fp16"], 3)
            recs.append(rec)
            del graphs, x, res, x_q, r_q
        torch.cuda.empty_cache()
    return recs


def step_model(a):
    import torch
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.centernet import CenterNet
    fp = CenterNet(seed=0).cuda().half()
    gen = torch.Generator().manual_seed(1)
    frame = torch.randn(SHAPES[0], generator=gen).cuda().half()
    q8, note8 = Q.build_int8_centernet(fp, torch.device("cuda"), [frame], calibrator="minmax_device", neck="int8")
    q16, note16 = Q.build_int8_centernet(fp, torch.device("cuda"), [frame], calibrator="minmax_device", neck="fp16")
    recs = []
    for shape in SHAPES:
        replays = a.replays if shape[0] == 1 else max(3, a.replays // 4)
        img = torch.randn(shape, generator=gen).cuda().half()
        outs = {"fp16": fp(img), "int8": q8(img), "int8_fp16neck": q16(img)}      # (eager: merged, packed, quantised operands)
        err = {k: [float((p.float() - f.float()).abs().max()) for p, f in zip(outs["fp16"], outs[k])]
               for k in ("int8", "int8_fp16neck")}
        del outs
        graphs = {"fp16": _capture(lambda: fp(img)), "int8": _capture(lambda: q8(img)),
                  "int8_fp16neck": _capture(lambda: q16(img))}
        ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, replays)
        rec = _summary({"step": "model", "workload": "CenterNet-R18-DCNv2 forward, HIP-graph replay, fp16 fast path vs the "
                        "INT8 builds (neck int8 / neck fp16)", "image": list(shape), "max_abs_diff_fp16_vs_int8": err,
                        "note_int8": note8, "note_int8_fp16neck": note16, "replays": replays,
                        "device": torch.cuda.get_device_name(0)}, ms)
        rec["int8_over_fp16"] = round(rec["median_ms_int8"] / rec["median_ms_fp16"], 3)
        rec["int8_fp16neck_over_fp16"] = round(rec["median_ms_int8_fp16neck"] / rec["median_ms_fp16"], 3)
        recs.append(rec)
        del graphs
        torch.cuda.empty_cache()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "centernet_int8"))
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
