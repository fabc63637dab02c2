#!/usr/bin/env python3
"""The INT8 BEV half of BEVDet-R50 (bevdet_int8.py) against the builds beside it.

  frame   the whole frame, HIP-graph replay, arms alternating in ONE process:
            int8_default   quantization.build_int8_bevdet(...)                  (int8 image chain + pooling, fp16 BEV half;
                           ranks as inputs: that model has no device index build)
            fp16_hip       BEVDet(bev_half="hip").forward_calibrated
            int8_bev       build_int8_bevdet(bev_half="int8").forward_calibrated
            int8_bev_ranks the same model with the ranks as inputs (the like-for-like partner of int8_default)
          and the BEV half alone through `bev_half_calibrated` (fp16_hip against int8_bev, each from its own image
          features).
  layers  every distinct convolution shape of the plan: `conv_slice_q_taps` on the operands one forward actually used,
          against the fp16 fast path's call for that layer (depth_net: dense_auto; the heads: conv_nhwc; everything else
          bevdet._conv under the rule dispatch) on random fp16 operands of the same shape.
  glue    the two launches of csrc/lss_split_s8.hip against their fp16 siblings (csrc/lss_split.hip) at the frame's
          shapes, with the bytes each moves and the share of the HBM peak (8 TB/s) that is.

Per alternation the mean of `--replays` replays between two events; median and maximum per arm over `--alternations`
(>= 5).  One JSON line per record, appended to <out-dir>/<step>.jsonl.  Every step is a child process of its own under
`timeout`; the script stops at the first step that fails.

    python tools/bevdet_int8_time.py [--alternations 7] [--replays 20] [--out-dir profiles/bevdet_int8]
    python tools/bevdet_int8_time.py --step layers      # one step, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from yolox_time import _alternate, _capture, _summary   # noqa: E402

STEPS = (("frame", 420), ("layers", 420), ("glue", 240))      # (name, seconds)
HBM_PEAK = 8.0e12                                             # bytes / s


def _models():
    """(fp16 "hip" model, default int8 model, int8-BEV-half model, image, ranks, calib): one state dict, one frame."""
    import torch
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.bevdet import BEVDet, synthetic_rig
    fp = BEVDet(seed=0, bev_half="hip").cuda().half()
    geom = synthetic_rig(fp.view)
    ranks = [r.cuda() for r in fp.view.get_bev_pool_input(*geom)]
    calib = fp.view.calibration_matrices(*geom).cuda()
    gen = torch.Generator().manual_seed(1)
    frame = (torch.randn(1, 6, 3, 256, 704, generator=gen).cuda().half(), *ranks)
    img = torch.randn(1, 6, 3, 256, 704, generator=gen).cuda().half()
    default, _, note_d = Q.build_int8_bevdet(fp, torch.device("cuda"), [frame], calibrator="minmax")
    q, _, note_q = Q.build_int8_bevdet(fp, torch.device("cuda"), [frame], calibrator="minmax", bev_half="int8")
    return fp, default, q, img, ranks, calib, note_d, note_q


def step_frame(a):
    import torch
    fp, default, q, img, ranks, calib, note_d, note_q = _models()
    dev = torch.cuda.get_device_name(0)
    arms = {"int8_default": lambda: default(img, *ranks), "fp16_hip": lambda: fp.forward_calibrated(img, calib),
            "int8_bev": lambda: q.forward_calibrated(img, calib), "int8_bev_ranks": lambda: q(img, *ranks)}
    outs = {k: [o.float() for o in f()] for k, f in arms.items()}       # (eager: merged, packed, quantised operands)
    err = {k: [float((p - r).abs().max()) for p, r in zip(outs[k], outs["fp16_hip"])] for k in arms if k != "fp16_hip"}
    del outs
    graphs = {k: _capture(f) for k, f in arms.items()}
    ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, a.replays)
    rec = _summary({"step": "frame", "workload": "BEVDet-R50 frame [1, 6, 3, 256, 704], HIP-graph replay", "device": dev,
                    "max_abs_diff_vs_fp16_hip": err, "note_int8_default": note_d, "note_int8_bev": note_q,
                    "replays": a.replays}, ms)
    for k in ("int8_bev", "int8_bev_ranks"):
        rec[f"{k}_over_int8_default"] = round(rec[f"median_ms_{k}"] / rec["median_ms_int8_default"], 3)
        rec[f"{k}_over_fp16_hip"] = round(rec[f"median_ms_{k}"] / rec["median_ms_fp16_hip"], 3)
    rec["fp16_hip_over_int8_bev"] = round(rec["median_ms_fp16_hip"] / rec["median_ms_int8_bev"], 3)
    recs = [rec]
    del graphs
    x16 = fp.image_features(img.flatten(0, 1)).clone()
    x8 = q._features(img).clone()
    halves = {"fp16_hip": lambda: fp.bev_half_calibrated(x16, calib), "int8_bev": lambda: q.bev_half_calibrated(x8, calib)}
    graphs = {k: _capture(f) for k, f in halves.items()}
    ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, a.replays)
    rec = _summary({"step": "frame", "workload": "BEVDet-R50 BEV half alone (bev_half_calibrated), HIP-graph replay",
                    "device": dev, "replays": a.replays}, ms)
    rec["int8_over_fp16"] = round(rec["median_ms_int8_bev"] / rec["median_ms_fp16_hip"], 3)
    recs.append(rec)
    return recs


class _ConvLog:
    """An operator set that forwards to functions and keeps the arguments of every conv_slice_q_taps call."""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __getattr__(self, name):
        return getattr(self.fn, name)

    def conv_slice_q_taps(self, *args, **kwargs):
        out = self.fn.conv_slice_q_taps(*args, **kwargs)
        self.calls.append((args, kwargs))
        return out


def step_layers(a):
    import torch
    import torch.nn as nn
    from bevformer_tensorrt_amd import bevdet as BD
    from bevformer_tensorrt_amd import functions as fn
    from bevformer_tensorrt_amd.functions import dispatch
    fp, default, q, img, ranks, calib, _, _ = _models()
    del default
    dev = torch.cuda.get_device_name(0)
    log = _ConvLog(fn)
    rb, rd, rf, ist, il = ranks
    pool = lambda d, f, s: fn.bev_pool_v2_int8(d, f, rd, rf, rb, ist, il, *s, 128, 128)   # noqa: E731
    q.prepare_bev_half()
    with dispatch.using(rule=True):
        q.run(q._features(img), pool, q.operands(), log)
    keys = [l.key for l in q.plan.layers if l.op == "conv"]
    seen, recs = {}, []
    g = torch.Generator().manual_seed(2)
    for key, (args, kwargs) in zip(keys, log.calls):
        x_q, sx, w, ws, b, act, res, sres, stride, _, sout, odt = args
        B, cin, H, W = x_q.shape
        cout, k = w.shape[0], w.shape[1]
        shape = (cin, cout, k, stride, H, W, act, res is not None, odt == torch.int8)
        if shape in seen:
            seen[shape]["launches_per_frame"] += 1
            seen[shape]["layers"].append(key)
            continue
        x16 = torch.randn(B, H, W, cin, generator=g).half().cuda().permute(0, 3, 1, 2)
        conv = nn.Conv2d(cin, cout, k, stride, k // 2).cuda().half()
        if k > 1:
            conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        r16 = None if res is None else torch.randn(B, Ho, Wo, cout, generator=g).half().cuda().permute(0, 3, 1, 2)
        relu = act == "relu"
        if key == "depth_net":
            rows, w2 = x16.permute(0, 2, 3, 1).reshape(-1, cin), conv.weight.detach().reshape(cout, cin)

            def fp16(rows=rows, w2=w2, conv=conv):
                with dispatch.using(rule=True):
                    return fn.dense_auto(rows, w2, conv.bias, None, False)
        elif key.startswith("head."):
            def fp16(x16=x16, conv=conv, relu=relu):
                with dispatch.using(rule=True):
                    return fn.conv_nhwc(x16, conv.weight, conv.bias, relu)
        else:
            def fp16(x16=x16, conv=conv, relu=relu, r16=r16):
                with dispatch.using(rule=True):
                    return BD._conv(fn, x16, conv, relu, r16)

        def int8(args=args, kwargs=kwargs):
            return fn.conv_slice_q_taps(*args[:9], None, *args[10:], **kwargs)
        graphs = {"fp16": _capture(fp16), "int8": _capture(int8)}
        ms = _alternate({n: v[0] for n, v in graphs.items()}, a.alternations, a.replays)
        rec = {"step": "layers", "layers": [key], "cin": cin, "cout": cout, "ksize": k, "stride": stride, "input_hw": [H, W],
               "batch": B, "act": act, "identity": res is not None, "out": "int8" if odt == torch.int8 else "fp16",
               "K": k * k * cin, "gflop": round(2.0 * B * Ho * Wo * k * k * cin * cout / 1e9, 3), "launches_per_frame": 1,
               "replays": a.replays, "device": dev}
        _summary(rec, ms)
        rec["int8_over_fp16"] = round(rec["median_ms_int8"] / rec["median_ms_fp16"], 3)
        seen[shape] = rec
        recs.append(rec)
        del graphs
    return recs


def step_glue(a):
    import torch
    from bevformer_tensorrt_amd import functions as fn
    dev = torch.cuda.get_device_name(0)
    g = torch.Generator().manual_seed(3)
    recs = []

    def record(name, arms, moved):
        graphs = {k: _capture(f) for k, f in arms.items()}
        ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, a.replays)
        rec = _summary({"step": "glue", "launch": name, "bytes_moved": moved, "replays": a.replays, "device": dev}, ms)
        for k in arms:
            rec[f"hbm_peak_share_{k}"] = round(moved[k] / (rec[f"median_ms_{k}"] * 1e-3) / HBM_PEAK, 4)
        rec["int8_over_fp16"] = round(rec["median_ms_int8"] / rec["median_ms_fp16"], 3)
        recs.append(rec)

    n, hw, D, C, stride = 6, 16 * 44, 59, 64, 128
    rows = (torch.randn(n * hw, stride, generator=g) * 3).half().cuda()
    record("depth softmax + split, 6 x 704 pixels, D = 59, C = 64",
           {"fp16": lambda: fn.lss_depth_split(rows, n, D, C, 64, 0), "int8": lambda: fn.lss_depth_split_q(rows, n, D, C, 64, 0, 1 / 127, 0.03)},
           {"fp16": n * hw * (D + C) * 4, "int8": n * hw * (D + C) * 3})
    for name, cb, hb, ca in (("bilinear x 4 into the 640-channel buffer, 16 x 16 x 512", 512, 16, 128), ("bilinear x 2, 64 x 64 x 512", 512, 64, 0)):
        f = 4 if ca else 2
        h = hb * f
        b16 = torch.randn(1, hb, hb, cb, generator=g).abs().half().cuda().permute(0, 3, 1, 2)
        a16 = torch.randn(1, h, h, ca, generator=g).half().cuda().permute(0, 3, 1, 2) if ca else None
        b8 = torch.randint(0, 128, (1, hb, hb, cb), generator=g, dtype=torch.int8).cuda().permute(0, 3, 1, 2)
        buf = torch.zeros(1, h, h, ca + cb, dtype=torch.int8, device="cuda").permute(0, 3, 1, 2)
        arms = {"fp16": (lambda a16=a16, b16=b16: fn.upsample_bilinear_concat_nhwc(a16, b16)) if ca else
                (lambda b16=b16: fn.upsample_bilinear_concat_nhwc(None, b16, scale_factor=2)),
                "int8": lambda b8=b8, buf=buf, ca=ca: fn.upsample_bilinear_nhwc_q(b8, 0.05, 0.037, out=buf[:, ca:])}
        # fp16: reads b and a, writes every channel (the concatenation's copy is part of the launch); int8: reads b, writes its slice
        record(name, arms, {"fp16": 2 * (hb * hb * cb + h * h * ca + h * h * (ca + cb)), "int8": hb * hb * cb + h * h * cb})
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "bevdet_int8"))
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
        recs = {"frame": step_frame, "layers": step_layers, "glue": step_glue}[a.step](a)
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
