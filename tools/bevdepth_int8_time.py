#!/usr/bin/env python3
"""The INT8 BEVDepth (bevdepth_int8.py) against the fp16 fast path of the parent commit, BEVDet(BEVDEPTH_R50,
bev_half="hip").

  frame   HIP-graph replay, arms alternating in ONE process:
            the whole frame          fp16_hip  BEVDet(BEVDEPTH_R50, "hip").forward_calibrated
                                     int8      build_int8_bevdet(<that model>, bev_half="int8").forward_calibrated
            DepthNet + split alone   fp16_hip  DepthNet.forward_hip + lss_depth_split
                                     int8      the plan's layers in front of the pooling (quantize pass included)
  layers  every distinct convolution shape of the DepthNet's plan, the three dilations and the per-image bias included:
          `conv_slice_q_taps` on the operands one forward actually used, against the fp16 fast path's call for that
          layer (conv_nhwc for reduce_conv and the BasicBlocks, conv_slice_nhwc for the rest) on random fp16 operands of
          the same shape.
  glue    the two launches of csrc/lss_depthnet_s8.hip against their fp16 siblings (csrc/lss_depthnet.hip) at the frame's
          shapes, with the bytes each moves and the share of the HBM peak (8 TB/s) that is.

Per alternation the mean of `--replays` replays between two events; median and maximum per arm over `--alternations`
(>= 5).  One JSON line per record, appended to <out-dir>/<step>.jsonl.  Every step is a child process of its own under
`timeout`; the script stops at the first step that fails.

    python tools/bevdepth_int8_time.py [--alternations 7] [--replays 20] [--out-dir profiles/bevdepth_int8]
    python tools/bevdepth_int8_time.py --step layers      # one step, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bevdet_int8_time import _ConvLog   # noqa: E402
from yolox_time import _alternate, _capture, _summary   # noqa: E402

STEPS = (("frame", 420), ("layers", 300), ("glue", 180))      # (name, seconds)
HBM_PEAK = 8.0e12                                             # bytes / s


def _models():
    """(fp16 "hip" BEVDepth model, its INT8 build, image, ranks, mlp_input, calib, note): one state dict, one frame."""
    import torch
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50, BEVDet, synthetic_rig
    fp = BEVDet(BEVDEPTH_R50, seed=0, bev_half="hip")
    geom = synthetic_rig(fp.view)
    v = fp.view.get_mlp_input(*geom).reshape(-1, 27)
    bn = fp.view.depth_net.bn               # (running statistics that fit the calibration values: the gates spread)
    with torch.no_grad():
        bn.running_mean.copy_(v.mean(0))
        bn.running_var.copy_((0.02 * v.abs().mean(0) + 0.05) ** 2)
    fp = fp.cuda().half()
    ranks = [r.cuda() for r in fp.view.get_bev_pool_input(*geom)]
    mlp = fp.view.get_mlp_input(*geom).cuda()
    calib = fp.view.calibration_matrices(*geom).cuda()
    gen = torch.Generator().manual_seed(1)
    frame = (torch.randn(1, 6, 3, 256, 704, generator=gen).cuda().half(), *ranks, mlp)
    img = torch.randn(1, 6, 3, 256, 704, generator=gen).cuda().half()
    q, _, note = Q.build_int8_bevdet(fp, torch.device("cuda"), [frame], calibrator="minmax", bev_half="int8")
    return fp, q, img, ranks, mlp, calib, note


def step_frame(a):
    import torch
    from bevformer_tensorrt_amd import functions as fn
    from bevformer_tensorrt_amd.functions import dispatch
    fp, q, img, ranks, mlp, calib, note = _models()
    dev = torch.cuda.get_device_name(0)
    arms = {"fp16_hip": lambda: fp.forward_calibrated(img, calib), "int8": lambda: q.forward_calibrated(img, calib)}
    outs = {k: [o.float() for o in f()] for k, f in arms.items()}
    err = [float((p - r).abs().max()) for p, r in zip(outs["int8"], outs["fp16_hip"])]
    del outs
    graphs = {k: _capture(f) for k, f in arms.items()}
    ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, a.replays)
    rec = _summary({"step": "frame", "workload": "BEVDepth-R50 frame [1, 6, 3, 256, 704], HIP-graph replay", "device": dev,
                    "max_abs_diff_vs_fp16_hip": err, "note_int8": note, "replays": a.replays}, ms)
    rec["int8_over_fp16_hip"] = round(rec["median_ms_int8"] / rec["median_ms_fp16_hip"], 3)
    recs = [rec]
    del graphs
    x16 = fp.image_features(img.flatten(0, 1)).clone()
    x8 = q._features(img).clone()
    m = mlp.reshape(-1, 27)
    view = fp.view
    table = q.operands()
    D, C = view.D, view.out_channels

    def fp16_front():
        with dispatch.using(rule=True):
            rows, lay = view.depth_net.forward_hip(x16, m, fn)
            return fn.lss_depth_split(rows, 6, D, C, lay["depth_offset"], lay["feat_offset"], spatial=x16.shape[2:])

    def int8_front():
        with dispatch.using(rule=True):
            return q.depth_and_features(x8, m, table, fn)

    fp16_front(), int8_front()
    graphs = {"fp16_hip": _capture(fp16_front), "int8": _capture(int8_front)}
    ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, a.replays)
    rec = _summary({"step": "frame", "workload": "BEVDepth-R50 DepthNet + softmax / split alone, HIP-graph replay",
                    "device": dev, "replays": a.replays}, ms)
    rec["int8_over_fp16_hip"] = round(rec["median_ms_int8"] / rec["median_ms_fp16_hip"], 3)
    recs.append(rec)
    return recs


def step_layers(a):
    import torch
    import torch.nn as nn
    from bevformer_tensorrt_amd import functions as fn
    from bevformer_tensorrt_amd.functions import dispatch
    fp, q, img, ranks, mlp, calib, _ = _models()
    dev = torch.cuda.get_device_name(0)
    log = _ConvLog(fn)
    rb, rd, rf, ist, il = ranks
    pool = lambda d, f, s: fn.bev_pool_v2_int8(d, f, rd, rf, rb, ist, il, *s, 128, 128)   # noqa: E731
    q.prepare_bev_half()
    with dispatch.using(rule=True):
        q.run(q._features(img), pool, q.operands(), log, mlp_input=mlp.reshape(-1, 27))
    front = [l for l in q.plan.layers[:q.plan.tail] if l.op == "conv"]
    seen, recs = {}, []
    g = torch.Generator().manual_seed(2)
    for l, (args, kwargs) in zip(front, log.calls):
        x_q, sx, w, ws, b, act, res, sres, stride, _, sout, odt = args
        d, ib = kwargs.get("dilation", 1), kwargs.get("image_bias")
        B, cin, H, W = x_q.shape
        cout, k = w.shape[0], w.shape[1]
        shape = (cin, cout, k, d, act, res is not None, ib is not None, odt == torch.int8)
        if shape in seen:
            seen[shape]["launches_per_frame"] += 1
            seen[shape]["layers"].append(l.key)
            continue
        x16 = torch.randn(B, H, W, cin, generator=g).half().cuda().permute(0, 3, 1, 2)
        conv = nn.Conv2d(cin, cout, k, 1, (k // 2) * d, d).cuda().half()
        if k > 1:
            conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
        r16 = None if res is None else torch.randn(B, H, W, cout, generator=g).half().cuda().permute(0, 3, 1, 2)
        ib16 = None if ib is None else torch.randn(B, cout, generator=g).half().cuda()
        relu = act == "relu"
        if k == 3 and d == 1:
            def fp16(x16=x16, conv=conv, relu=relu, r16=r16):
                with dispatch.using(rule=True):
                    return fn.conv_nhwc(x16, conv.weight, conv.bias, relu, r16)
        else:
            def fp16(x16=x16, conv=conv, act=act, d=d, ib16=ib16):
                with dispatch.using(rule=True):
                    return fn.conv_slice_nhwc(x16, conv.weight, None if ib16 is not None else conv.bias, act, dilation=d,
                                              image_bias=ib16)

        def int8(args=args, kwargs=kwargs):
            return fn.conv_slice_q_taps(*args[:9], None, *args[10:], **kwargs)
        fp16(), int8()
        graphs = {"fp16": _capture(fp16), "int8": _capture(int8)}
        ms = _alternate({n: v[0] for n, v in graphs.items()}, a.alternations, a.replays)
        rec = {"step": "layers", "layers": [l.key], "cin": cin, "cout": cout, "ksize": k, "dilation": d, "input_hw": [H, W],
               "batch": B, "act": act, "identity": res is not None, "image_bias": ib is not None,
               "out": "int8" if odt == torch.int8 else "fp16", "K": k * k * cin,
               "gflop": round(2.0 * B * H * W * k * k * cin * cout / 1e9, 3), "launches_per_frame": 1, "replays": a.replays,
               "device": dev}
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
        for f in arms.values():
            f()
        graphs = {k: _capture(f) for k, f in arms.items()}
        ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, a.replays)
        rec = _summary({"step": "glue", "launch": name, "bytes_moved": moved, "replays": a.replays, "device": dev}, ms)
        for k in arms:
            rec[f"hbm_peak_share_{k}"] = round(moved[k] / (rec[f"median_ms_{k}"] * 1e-3) / HBM_PEAK, 4)
        rec["int8_over_fp16"] = round(rec["median_ms_int8"] / rec["median_ms_fp16"], 3)
        recs.append(rec)

    n, H, W, c = 6, 16, 44, 256
    x16 = torch.randn(n, H, W, c, generator=g).half().cuda().permute(0, 3, 1, 2)
    x8 = torch.randint(-127, 128, (n, H, W, c), generator=g, dtype=torch.int8).cuda().permute(0, 3, 1, 2)
    gates = torch.rand(2, n, c, generator=g).cuda()
    px = n * H * W * c
    record("both gated copies, 6 x 704 pixels x 256 channels",
           {"fp16": lambda: fn.se_gate2_nhwc(x16, gates), "int8": lambda: fn.se_gate2_nhwc_q(x8, 0.03, gates, 0.02, 0.025)},
           {"fp16": px * 2 * 3, "int8": px * 3})
    record("global average pool, 6 x 704 pixels x 256 channels",
           {"fp16": lambda: fn.global_avgpool_nhwc(x16), "int8": lambda: fn.global_avgpool_nhwc_q(x8, 0.03)},
           {"fp16": px * 2, "int8": px})
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "bevdepth_int8"))
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
