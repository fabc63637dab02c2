#!/usr/bin/env python3
"""INT8 YOLOX-Nano (quantization.build_int8_yolox(depthwise="int8")): the int8 depthwise-separable launch against the
fp16 one on every distinct layer shape, and the INT8 forward against the fp16 fast path.

  layers  every distinct (Cin, Cout, stride, map, identity) of one forward (tools/yolox_depthwise_time.py's list):
            int8   `dwsep_conv_q_taps` (csrc/dwsep_conv_s8.hip), int8 in, int8 out, per-channel scales, SiLU twice
            fp16   `dwsep_conv_taps` (csrc/dwsep_conv.hip) on the same shape
          with the bytes the int8 launch must move and the share of the HBM peak (8 TB/s) its median amounts to.  Every
          shape is reported, the slower ones too: no ratio is a gate or a dispatch rule.
  model   `Int8YOLOX.forward` against `YOLOX.forward` on the fp16 fast path, the same weights (min-max, two frames)

HIP-graph replay, the arms of one record in ONE process and replayed alternately; median and maximum per arm over the
alternations (tools/yolox_time.py's routines).  Image shapes (1, 3, 416, 416) and (32, 3, 416, 416).  One JSON line per
record, appended to <out-dir>/<step>.jsonl; every step is a child process of its own under `timeout`.

    python tools/yolox_depthwise_int8_time.py [--alternations 7] [--replays 20] [--out-dir profiles/yolox_depthwise_int8]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from yolox_time import _alternate, _capture, _summary   # noqa: E402
from yolox_depthwise_time import PEAK_HBM_TBS, SHAPES, _layer_list   # noqa: E402

STEPS = (("layers", 420), ("model", 300))      # (name, seconds)


def step_layers(a):
    import torch
    from bevformer_tensorrt_amd import functions as ops
    from bevformer_tensorrt_amd.functions.yolox_ops import nhwc_empty
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_NANO
    g = torch.Generator().manual_seed(0)
    dev = torch.cuda.get_device_name(0)
    model = YOLOX(YOLOX_NANO, seed=0).cuda().half()
    recs = []
    for shape in SHAPES:
        B = shape[0]
        replays = a.replays if B == 1 else max(3, a.replays // 4)
        for (cin, cout, stride, h, w, idt), count in _layer_list(model, shape).items():
            ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
            xf = torch.randn(B, cin, h, w, generator=g)
            wd, wp = torch.randn(cin, 1, 3, 3, generator=g) / 3.0, torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
            bd, bp = torch.randn(cin, generator=g), torch.randn(cout, generator=g)
            rf = torch.randn(B, cout, ho, wo, generator=g) if idt else None
            # fp16 arm
            x16 = nhwc_empty(B, cin, h, w, "cuda")
            x16.copy_(xf)
            taps, pw = ops.dwsep_conv_packed_weight(wd.half().cuda(), wp.half().cuda(), cin, cout)
            bd16, bp16 = bd.half().cuda(), bp.half().cuda()
            r16 = None
            if idt:
                r16 = nhwc_empty(B, cout, ho, wo, "cuda")
                r16.copy_(rf)
            # int8 arm: the same layer quantised, activations at 4 sigma / 127
            q = [t.cuda() for t in ops.quantize_dwsep_weights(wd, bd, wp, bp, cin, cout)]
            sx = st = so = sr = 4.0 / 127.0
            x8 = nhwc_empty(B, cin, h, w, "cuda", torch.int8)
            x8.copy_(torch.clamp(torch.round(xf / sx), -127, 127))
            r8 = None
            if idt:
                r8 = nhwc_empty(B, cout, ho, wo, "cuda", torch.int8)
                r8.copy_(torch.clamp(torch.round(rf / sr), -127, 127))

            def fp16():
                return ops.dwsep_conv_taps(x16, taps, bd16, pw, bp16, "silu", "silu", r16, stride)

            def int8():
                return ops.dwsep_conv_q_taps(x8, sx, q[0], q[1], q[2], st, q[3], q[4], q[5], "silu", "silu", r8, sr, stride,
                                             None, so)
            graphs = {"fp16": _capture(fp16), "int8": _capture(int8)}
            ms = _alternate({n: v[0] for n, v in graphs.items()}, a.alternations, replays)
            nbytes = x8.numel() + B * ho * wo * cout * (2 if idt else 1) + 9 * cin + 8 * cin + cout * cin + 8 * cout
            rec = {"step": "layers", "layer": f"dwsep {cin} -> {cout} 3x3 / {stride} silu{' + identity' if idt else ''}",
                   "input": [B, cin, h, w], "image": list(shape), "launches_per_forward": count,
                   "mbytes_int8": round(nbytes / 1e6, 3), "replays": replays, "device": dev}
            _summary(rec, ms)
            rec["tbs_int8"] = round(nbytes / 1e9 / rec["median_ms_int8"], 3)
            rec["fraction_of_hbm_peak_int8"] = round(rec["tbs_int8"] / PEAK_HBM_TBS, 4)
            rec["int8_over_fp16"] = round(rec["median_ms_int8"] / rec["median_ms_fp16"], 3)
            recs.append(rec)
            del graphs
        torch.cuda.empty_cache()
    return recs


def step_model(a):
    import torch
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_NANO
    fp = YOLOX(YOLOX_NANO, seed=0).cuda().half()
    g = torch.Generator().manual_seed(1)
    frames = [torch.randn((1, 3, 416, 416), generator=g).cuda().half() for _ in range(2)]
    q, note = Q.build_int8_yolox(fp, torch.device("cuda"), frames, calibrator="minmax", depthwise="int8")
    q.prepare()
    recs = []
    for shape in SHAPES:
        replays = a.replays if shape[0] == 1 else max(3, a.replays // 4)
        img = torch.randn(shape, generator=g).cuda().half()
        err = [float((p.float() - f.float()).abs().max()) for p, f in zip(fp(img), q(img))]
        graphs = {"fp16": _capture(lambda: fp(img)), "int8": _capture(lambda: q(img))}
        ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, replays)
        rec = _summary({"step": "model", "workload": "YOLOX-Nano forward, HIP-graph replay, int8 build against fp16 fast path",
                        "image": list(shape), "note": note, "max_abs_diff_fp16_vs_int8": err, "replays": replays,
                        "device": torch.cuda.get_device_name(0)}, ms)
        rec["int8_over_fp16"] = round(rec["median_ms_int8"] / rec["median_ms_fp16"], 3)
        recs.append(rec)
        del graphs
        torch.cuda.empty_cache()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "yolox_depthwise_int8"))
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
