#!/usr/bin/env python3
"""The INT8 form of the DepthNet's DCN layer (csrc/deform_conv_s8.hip, build_int8_bevdet(depthnet_dcn="int8")) against
its fp16 form and against the INT8 BEVDepth without the layer.

  op      HIP-graph replay, arms alternating in ONE process:
            the deformable launch    fp16  bevops_deform_conv3x3_nhwc_f16 (deform_conv2d_nhwc)
                                     int8  bevops_deform_conv3x3_nhwc_s8  (deform_conv2d_q_nhwc, int8 out)
                                     at (6, 256, 16, 44) and (48, 256, 16, 44), groups 4, Gaussian offsets of one pixel,
                                     both reading the SAME fp16 offset rows
            the offset convolution   fp16  conv_offset_nhwc (256 -> 32 rows)
                                     int8  conv_slice_q_taps 3 x 3, 256 -> 24 rows, fp16 out
  frame   the whole frame and DepthNet + softmax / split alone:
            fp16_dcn   BEVDet(BEVDEPTH_R50_DCN, "hip"): the fp16 fast path with the layer
            int8_dcn   its INT8 build with depthnet_dcn="int8"
            int8       the INT8 build of BEVDEPTH_R50 (no layer) on the weights both models share
          with the error figures of the INT8 build: max |int8_dcn - fp16_dcn| per head output.

Per alternation the mean of `--replays` replays between two events; median and maximum per arm over `--alternations`
(>= 5).  One JSON line per record, appended to <out-dir>/<step>.jsonl.  Every step is a child process of its own under
`timeout`; the script stops at the first step that fails.

    python tools/bevdepth_dcn_int8_time.py [--alternations 7] [--replays 20] [--out-dir profiles/bevdepth_dcn_int8]
    python tools/bevdepth_dcn_int8_time.py --step op      # one step, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from yolox_time import _alternate, _capture, _summary   # noqa: E402

STEPS = (("op", 240), ("frame", 480))                   # (name, seconds)


def step_op(a):
    import torch
    from bevformer_tensorrt_amd import functions as fn
    from bevformer_tensorrt_amd.functions import yolox_ops as Y
    dev = torch.cuda.get_device_name(0)
    g = torch.Generator().manual_seed(7)
    C, G, H, W = 256, 4, 16, 44
    recs = []

    def record(what, B, arms, extra):
        for f in arms.values():
            f()
        graphs = {k: _capture(f) for k, f in arms.items()}
        ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, a.replays)
        rec = _summary(dict({"step": "op", "launch": what, "shape": [B, C, H, W], "groups": G, "replays": a.replays,
                             "device": dev}, **extra), ms)
        rec["int8_over_fp16"] = round(rec["median_ms_int8"] / rec["median_ms_fp16"], 3)
        recs.append(rec)

    weight = (torch.randn(C, C // G, 3, 3, generator=g) * 0.05).half().cuda()
    wq, ws, _ = Y.quantize_weight_taps(weight, None)
    ow = (torch.randn(18, C, 3, 3, generator=g) * 0.02).half().cuda()
    ob = (torch.randn(18, generator=g) * 0.3).half().cuda()
    owq, ows, obq = Y.quantize_weight_taps(ow, ob, multiple=8)
    for B in (6, 48):
        x16 = torch.randn(B, H, W, C, generator=g).half().cuda().permute(0, 3, 1, 2)
        x8 = torch.randint(-127, 128, (B, H, W, C), generator=g, dtype=torch.int8).cuda().permute(0, 3, 1, 2)
        om = torch.randn(B, H, W, 32, generator=g).half().cuda().permute(0, 3, 1, 2)       # sigma one pixel
        corners = B * H * W * 9 * 4 * C                                                    # elements gathered
        record("deformable convolution", B,
               {"fp16": lambda: fn.deform_conv2d_nhwc(x16, om, weight, None, G),
                "int8": lambda: fn.deform_conv2d_q_nhwc(x8, 0.03, om, wq, ws, None, G, scale_out=0.05)},
               {"corner_bytes_fp16": corners * 2, "corner_bytes_int8": corners,
                "gflop": round(2.0 * B * H * W * 9 * (C // G) * C / 1e9, 3)})
        record("offset convolution", B,
               {"fp16": lambda: fn.conv_offset_nhwc(x16, ow, ob),
                "int8": lambda: fn.conv_slice_q_taps(x8, 0.03, owq, ows, obq, "none", out_dtype=torch.float16)},
               {"rows_fp16": 32, "rows_int8": 24})
    return recs


def _models():
    """(fp16 "hip" model with the layer, its INT8 build, the INT8 build of the model without the layer, image, mlp_input,
    calib, notes): shared weights, conv_offset set to offsets of about one pixel."""
    import torch
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50, BEVDEPTH_R50_DCN, BEVDet, synthetic_rig
    fp = BEVDet(BEVDEPTH_R50_DCN, seed=0, bev_half="hip")
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
    # offsets of about one pixel: scale conv_offset by what the fp16 fast path shows on this frame
    dcn = fp.view.depth_net.dcn
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        dcn.conv_offset.weight.copy_((torch.randn(18, 256, 3, 3, generator=g) * 0.02).to(dcn.conv_offset.weight))
        dcn.conv_offset.bias.copy_((torch.randn(18, generator=g) * 0.3).to(dcn.conv_offset.bias))
    seen = []
    inner = dcn.forward_hip

    def probe(x, ops):
        seen.append(float(ops.conv_offset_nhwc(x, dcn.conv_offset.weight, dcn.conv_offset.bias)[:, :18].float().std()))
        return inner(x, ops)

    dcn.forward_hip = probe
    try:
        with torch.no_grad():
            fp.forward_calibrated(img, calib)
    finally:
        del dcn.forward_hip
    with torch.no_grad():
        dcn.conv_offset.weight.mul_(1.0 / seen[0])
        dcn.conv_offset.bias.mul_(1.0 / seen[0])
    dev = torch.device("cuda")
    q, _, note = Q.build_int8_bevdet(fp, dev, [frame], calibrator="minmax", bev_half="int8", depthnet_dcn="int8")
    plain = BEVDet(BEVDEPTH_R50, seed=0, bev_half="hip").cuda().half()
    sd = {k: v for k, v in fp.state_dict().items() if ".depth_conv.4." not in k and ".depth_conv.5." not in k}
    sd.update({k.replace(".depth_conv.5.", ".depth_conv.4."): v for k, v in fp.state_dict().items() if ".depth_conv.5." in k})
    plain.load_state_dict(sd)
    q0, _, note0 = Q.build_int8_bevdet(plain, dev, [frame], calibrator="minmax", bev_half="int8")
    return fp, q, q0, img, mlp, calib, {"int8_dcn": note, "int8": note0, "offset_std_before_scaling": seen[0]}


def step_frame(a):
    import torch
    from bevformer_tensorrt_amd import functions as fn
    from bevformer_tensorrt_amd.functions import dispatch
    fp, q, q0, img, mlp, calib, notes = _models()
    dev = torch.cuda.get_device_name(0)
    arms = {"fp16_dcn": lambda: fp.forward_calibrated(img, calib), "int8_dcn": lambda: q.forward_calibrated(img, calib),
            "int8": lambda: q0.forward_calibrated(img, calib)}
    outs = {k: [o.float() for o in f()] for k, f in arms.items()}
    err = [float((p - r).abs().max()) for p, r in zip(outs["int8_dcn"], outs["fp16_dcn"])]
    del outs
    graphs = {k: _capture(f) for k, f in arms.items()}
    ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, a.replays)
    rec = _summary({"step": "frame", "workload": "BEVDepth-R50 + DCN frame [1, 6, 3, 256, 704], HIP-graph replay",
                    "device": dev, "max_abs_diff_int8_dcn_vs_fp16_dcn": err, "notes": notes, "replays": a.replays}, ms)
    rec["int8_dcn_over_fp16_dcn"] = round(rec["median_ms_int8_dcn"] / rec["median_ms_fp16_dcn"], 3)
    rec["int8_dcn_over_int8"] = round(rec["median_ms_int8_dcn"] / rec["median_ms_int8"], 3)
    recs = [rec]
    del graphs
    x16 = fp.image_features(img.flatten(0, 1)).clone()
    x8, x80 = q._features(img).clone(), q0._features(img).clone()
    m = mlp.reshape(-1, 27)
    view = fp.view
    t, t0 = q.operands(), q0.operands()
    D, C = view.D, view.out_channels

    def fp16_front():
        with dispatch.using(rule=True):
            rows, lay = view.depth_net.forward_hip(x16, m, fn)
            return fn.lss_depth_split(rows, 6, D, C, lay["depth_offset"], lay["feat_offset"], spatial=x16.shape[2:])

    def int8_dcn_front():
        with dispatch.using(rule=True):
            return q.depth_and_features(x8, m, t, fn)

    def int8_front():
        with dispatch.using(rule=True):
            return q0.depth_and_features(x80, m, t0, fn)

    fronts = {"fp16_dcn": fp16_front, "int8_dcn": int8_dcn_front, "int8": int8_front}
    for f in fronts.values():
        f()
    graphs = {k: _capture(f) for k, f in fronts.items()}
    ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, a.replays)
    rec = _summary({"step": "frame", "workload": "BEVDepth-R50 + DCN DepthNet + softmax / split alone, HIP-graph replay",
                    "device": dev, "replays": a.replays}, ms)
    rec["int8_dcn_over_fp16_dcn"] = round(rec["median_ms_int8_dcn"] / rec["median_ms_fp16_dcn"], 3)
    rec["int8_dcn_over_int8"] = round(rec["median_ms_int8_dcn"] / rec["median_ms_int8"], 3)
    recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "bevdepth_dcn_int8"))
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
        recs = {"op": step_op, "frame": step_frame}[a.step](a)
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
