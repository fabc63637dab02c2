#!/usr/bin/env python3
"""INT8 YOLOX-x (yolox_int8.py) against the fp16 fast path (yolox.py): every distinct convolution shape, and the whole
forward.

  layers  every distinct (Cin, Cout, k, stride, map, activation, identity, output type) of one YOLOX-x forward, as both
          paths launch it (padded widths, stacked / block-diagonal head operands): `conv_slice_q_taps`
          (csrc/conv_slice_s8.hip; int8 in, int8 out, fp16 out for the packed predictors) against `conv_slice_taps`
          (csrc/conv_slice.hip, fp16 in and out).  Dense operands on both sides (pitch == channels).
  model   `Int8YOLOX.forward` against `YOLOX.forward` (fast path) on the same weights; the int8 model is calibrated on
          one random frame with the device min-max calibrator (the scales do not change the time).

Both under HIP-graph replay, both arms in ONE process, replayed alternately (fp16, int8, fp16, int8, ...): per
alternation the mean of `--replays` replays between two events; median and maximum per arm over `--alternations` (>= 5)
alternations.  Image shapes: (1, 3, 640, 640) and the reference's engine shape (32, 3, 640, 640).

One JSON line per record, appended to <out-dir>/<step>.jsonl.  Every step is a child process of its own under `timeout`;
the script stops at the first step that fails.

    python tools/yolox_int8_time.py [--alternations 7] [--replays 20] [--out-dir profiles/yolox_int8]
    python tools/yolox_int8_time.py --step layers      # one step, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from yolox_time import SHAPES, _alternate, _capture, _summary   # noqa: E402

STEPS = (("layers", 560), ("model", 420))      # (name, seconds)


def _layer_list(model):
    """The distinct convolution launches of the plan, in first-use order, with their counts:
    {(Cin, Cout, k, stride, div, act, identity, fp16 out): count}; div: the image's size over the input map's."""
    seen = {}
    table = model.operands()
    for s in model.plan.steps:
        if s.op != "conv":
            continue
        k = table[s.key][0].shape[1]
        key = (s.src.C, s.dst.C, k, s.stride, s.src.div, s.act, s.res is not None, model.plan.bufs[s.dst.buf][2] == "f16")
        seen[key] = seen.get(key, 0) + 1
    return seen


def step_layers(a):
    import torch
    from bevformer_tensorrt_amd import functions as ops
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_X
    from bevformer_tensorrt_amd.yolox_int8 import Int8YOLOX, build_plan
    g = torch.Generator().manual_seed(0)
    dev = torch.cuda.get_device_name(0)
    fp = YOLOX(YOLOX_X, seed=0).cuda().half()
    model = Int8YOLOX(fp, [1.0] * build_plan(fp).groups()[1])
    layers = _layer_list(model)
    recs = []
    for shape in SHAPES:
        B = shape[0]
        replays = a.replays if B == 1 else max(3, a.replays // 4)
        for (cin, cout, k, stride, div, act, idt, f16_out), count in layers.items():
            h, w = shape[2] // div, shape[3] // div
            ho, wo = (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1
            nhwc = lambda t: t.contiguous(memory_format=torch.channels_last)    # noqa: E731
            x = nhwc(torch.randn(B, cin, h, w, generator=g).half().cuda())
            wt = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).half()
            taps = wt.permute(0, 2, 3, 1).contiguous().cuda()
            bias = torch.randn(cout, generator=g).half().cuda()
            res = nhwc(torch.randn(B, cout, ho, wo, generator=g).half().cuda()) if idt else None
            # unit-normal activations and identities clip beyond 5 sigma, the output (conv + bias + identity) beyond 12
            sx, sr, so = 5.0 / 127, 5.0 / 127, 12.0 / 127
            x_q = nhwc(torch.clamp(torch.round(x.float() / sx), -127, 127).to(torch.int8))
            r_q = nhwc(torch.clamp(torch.round(res.float() / sr), -127, 127).to(torch.int8)) if idt else None
            wq, ws, b32 = (t.cuda() for t in ops.quantize_weight_taps(wt, bias.cpu(), multiple=8))
            odt = torch.float16 if f16_out else torch.int8

            def fp16(x=x, taps=taps, bias=bias, res=res, act=act, stride=stride):
                return ops.conv_slice_taps(x, taps, bias, act, res, stride)

            def int8(x_q=x_q, wq=wq, ws=ws, b32=b32, r_q=r_q, act=act, stride=stride, odt=odt):
                return ops.conv_slice_q_taps(x_q, sx, wq, ws, b32, act, r_q, sr, stride, None, None if f16_out else so, odt)
            y16, y8 = fp16().float(), int8().float() * (1.0 if f16_out else so)
            err = float((y16 - y8).abs().max())
            graphs = {"fp16": _capture(fp16), "int8": _capture(int8)}
            ms = _alternate({n: v[0] for n, v in graphs.items()}, a.alternations, replays)
            gflop = 2.0 * B * ho * wo * k * k * cin * cout / 1e9
            mbytes_fp16 = (x.numel() + y16.numel() + (res.numel() if idt else 0)) * 2 / 1e6
            rec = {"step": "layers", "layer": f"conv {cin} -> {cout} {k}x{k} / {stride} {act}{' + identity' if idt else ''}"
                   f"{' -> fp16' if f16_out else ''}", "input": [B, cin, h, w], "image": list(shape),
                   "launches_per_forward": count, "gflop": round(gflop, 3), "activation_mbytes_fp16": round(mbytes_fp16, 2),
                   "max_abs_diff_fp16_vs_int8": err, "replays": replays, "device": dev}
            _summary(rec, ms)
            rec["tops_int8"] = round(gflop / rec["median_ms_int8"], 1)
            rec["tflops_fp16"] = round(gflop / rec["median_ms_fp16"], 1)
            rec["int8_over_fp16"] = round(rec["median_ms_int8"] / rec["median_ms_fp16"], 3)
            recs.append(rec)
            del graphs, x, res, x_q, r_q
        torch.cuda.empty_cache()
    return recs


def step_model(a):
    import torch
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_X
    fp = YOLOX(YOLOX_X, seed=0).cuda().half()
    gen = torch.Generator().manual_seed(1)
    frame = torch.randn(SHAPES[0], generator=gen).cuda().half()
    q, note = Q.build_int8_yolox(fp, torch.device("cuda"), [frame], calibrator="minmax_device")
    recs = []
    for shape in SHAPES:
        replays = a.replays if shape[0] == 1 else max(3, a.replays // 4)
        img = torch.randn(shape, generator=gen).cuda().half()
        outs = {"fp16": fp(img), "int8": q(img)}                  # (eager: merged, padded and quantised operands)
        err = [float((p.float() - f.float()).abs().max()) for p, f in zip(outs["fp16"], outs["int8"])]
        del outs
        graphs = {"fp16": _capture(lambda: fp(img)), "int8": _capture(lambda: q(img))}
        ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, replays)
        rec = _summary({"step": "model", "workload": "YOLOX-x forward, HIP-graph replay, fp16 fast path vs INT8 build",
                        "image": list(shape), "max_abs_diff_fp16_vs_int8": err, "note": note, "replays": replays,
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
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "yolox_int8"))
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
