#!/usr/bin/env python3
"""YOLOX-Nano (yolox.YOLOX_NANO, use_depthwise): every distinct depthwise-separable layer shape of its fast path in three
forms, and the whole fast path against the plain fp16 path.

  layers  every distinct (Cin, Cout, stride, map, identity) of one forward as the fast path launches it (padded widths):
            fused    `dwsep_conv_taps` (csrc/dwsep_conv.hip), one launch
            two      F.conv2d(groups=C) on channels-last fp16 + a SiLU pass, then `conv_slice_taps` 1x1 (SiLU and the
                     identity in its epilogue): the form the fast path would have had without the new kernel
            library  F.conv2d(groups=C) + SiLU pass + F.conv2d 1x1 + SiLU pass (+ identity add)
          with the bytes the fused launch must move (x, out and the identity once, the weights once) and the share of
          the HBM peak (8 TB/s, the data sheet's figure) that its median time amounts to.
  model   `YOLOX.forward` on the fast path against the plain path on the same fp16 state dict

HIP-graph replay, the arms of one record in ONE process and replayed alternately; median and maximum per arm over the
alternations (tools/yolox_time.py's routines).  Image shapes (1, 3, 416, 416) and (32, 3, 416, 416).  One JSON line per
record, appended to <out-dir>/<step>.jsonl; every step is a child process of its own under `timeout`.

    python tools/yolox_depthwise_time.py [--alternations 7] [--replays 20] [--out-dir profiles/yolox_depthwise]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from yolox_time import _alternate, _capture, _summary   # noqa: E402

STEPS = (("layers", 540), ("model", 300))      # (name, seconds)
SHAPES = ((1, 3, 416, 416), (32, 3, 416, 416))
PEAK_HBM_TBS = 8.0


def _layer_list(model, shape):
    """{(Cin, Cout, stride, H, W, identity): count} of the dwsep_conv_taps launches of one fast forward."""
    import types
    import torch
    import bevformer_tensorrt_amd.functions as fn
    seen = {}

    def probe(x, wd, bd, wp, bp, act_dw="silu", act_pw="silu", residual=None, stride=1, out=None):
        key = (x.shape[1], wp.shape[0], stride, x.shape[2], x.shape[3], residual is not None)
        seen[key] = seen.get(key, 0) + 1
        return fn.dwsep_conv_taps(x, wd, bd, wp, bp, act_dw, act_pw, residual, stride, out)

    ops = types.SimpleNamespace(**{n: getattr(fn, n) for n in fn.__all__})
    ops.dwsep_conv_taps = probe
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
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_NANO
    g = torch.Generator().manual_seed(0)
    dev = torch.cuda.get_device_name(0)
    model = YOLOX(YOLOX_NANO, seed=0).cuda().half()
    cl = lambda t: t.half().cuda().contiguous(memory_format=torch.channels_last)      # noqa: E731
    recs = []
    for shape in SHAPES:
        B = shape[0]
        replays = a.replays if B == 1 else max(3, a.replays // 4)
        for (cin, cout, stride, h, w, idt), count in _layer_list(model, shape).items():
            x = cl(torch.randn(B, cin, h, w, generator=g))
            wd = (torch.randn(cin, 1, 3, 3, generator=g) / 3.0).half().cuda()
            wp = (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).half().cuda()
            bd, bp = torch.randn(cin, generator=g).half().cuda(), torch.randn(cout, generator=g).half().cuda()
            taps, pw = ops.dwsep_conv_packed_weight(wd, wp, cin, cout)
            pw_taps = wp.permute(0, 2, 3, 1).contiguous()
            ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
            res = cl(torch.randn(B, cout, ho, wo, generator=g)) if idt else None

            def depthwise():
                t = F.conv2d(x, wd, bd, stride, 1, 1, cin)
                return t * torch.sigmoid(t)

            def library():
                y = F.conv2d(depthwise(), wp, bp)
                y = y * torch.sigmoid(y)
                return y if res is None else y + res

            def two():
                return ops.conv_slice_taps(depthwise(), pw_taps, bp, "silu", res, 1)

            def fused():
                return ops.dwsep_conv_taps(x, taps, bd, pw, bp, "silu", "silu", res, stride)
            err = float((library().float() - fused().float()).abs().max())
            graphs = {"library": _capture(library), "two": _capture(two), "fused": _capture(fused)}
            ms = _alternate({n: v[0] for n, v in graphs.items()}, a.alternations, replays)
            nbytes = 2 * (x.numel() + B * ho * wo * cout * (2 if idt else 1) + 10 * cin + cout * cin + cout)
            rec = {"step": "layers", "layer": f"dwsep {cin} -> {cout} 3x3 / {stride} silu{' + identity' if idt else ''}",
                   "input": [B, cin, h, w], "image": list(shape), "launches_per_forward": count, "mbytes_fused": round(nbytes / 1e6, 3),
                   "max_abs_diff_library_vs_fused": err, "replays": replays, "device": dev}
            _summary(rec, ms)
            rec["tbs_fused"] = round(nbytes / 1e9 / rec["median_ms_fused"], 3)
            rec["fraction_of_hbm_peak_fused"] = round(rec["tbs_fused"] / PEAK_HBM_TBS, 4)
            rec["fused_over_two"] = round(rec["median_ms_fused"] / rec["median_ms_two"], 3)
            rec["fused_over_library"] = round(rec["median_ms_fused"] / rec["median_ms_library"], 3)
            recs.append(rec)
            del graphs, x, res
        torch.cuda.empty_cache()
    return recs


def step_model(a):
    import types
    import torch
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_NANO
    fast = YOLOX(YOLOX_NANO, seed=0).cuda().half()
    plain = YOLOX(YOLOX_NANO, seed=0, ops=types.SimpleNamespace()).cuda().half()
    plain.load_state_dict(fast.state_dict())
    recs = []
    for shape in SHAPES:
        replays = a.replays if shape[0] == 1 else max(3, a.replays // 4)
        img = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda().half()
        err = [float((p.float() - f.float()).abs().max()) for p, f in zip(plain(img), fast(img))]
        graphs = {"plain": _capture(lambda: plain(img)), "fast": _capture(lambda: fast(img))}
        ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, replays)
        recs.append(_summary({"step": "model", "workload": "YOLOX-Nano forward, HIP-graph replay, fp16",
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
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "yolox_depthwise"))
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
