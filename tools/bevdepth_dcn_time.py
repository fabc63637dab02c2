#!/usr/bin/env python3
"""The DepthNet's DCN layer (grouped, unmodulated deformable convolution; csrc/deform_conv.hip) on one MI355X, under
HIP-graph replay, arms replayed alternately.

  op        deform_conv2d_nhwc (ONE launch for the four groups, offsets read from the offset convolution's rows) against
            modulated_deformable_conv2d_nhwc with planar offsets and a ones mask (one launch per group), at
            (6, 256, 16, 44) and (48, 256, 16, 44), 256 -> 256 channels, groups 4; the permute to planar offsets and the
            ones tensor are made outside the timed region.  And the offset convolution (conv_offset_nhwc) alone.
  depthnet  LSSViewTransformerBEVDepth._depth_feat (DepthNet + softmax / split) on fixed image features,
            BEVDEPTH_R50_DCN against BEVDEPTH_R50
  frame     BEVDet.forward_calibrated, BEVDEPTH_R50_DCN against BEVDEPTH_R50

Per alternation the mean of `--replays` replays between two events; median and maximum per arm.  One JSON line per
record, appended to profiles/bevdepth_dcn/<step>.jsonl.  Every step is a child process of its own under `timeout`; the
script stops at the first step that fails.  No ratio here is a gate: the records say what was measured.

    python tools/bevdepth_dcn_time.py [--alternations 7] [--replays 20] [--out-dir profiles/bevdepth_dcn]
    python tools/bevdepth_dcn_time.py --step op      # one step, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bevdepth_time import _alternate, _capture, _record      # noqa: E402  (the protocol of tools/bevdepth_time.py)

STEPS = (("op", 300), ("depthnet", 300), ("frame", 420))      # (name, seconds)


def step_op(a):
    import torch
    import bevformer_tensorrt_amd as bev
    g = torch.Generator().manual_seed(0)
    cl = torch.channels_last
    recs = []
    for n in (6, 48):
        c, H, W, G = 256, 16, 44, 4
        x = torch.randn(n, c, H, W, generator=g).cuda().half().contiguous(memory_format=cl)
        w = (torch.randn(c, c // G, 3, 3, generator=g) / (9 * c // G) ** 0.5).cuda().half()
        wo = (torch.randn(18, c, 3, 3, generator=g) * 0.01).cuda().half()
        bo = torch.randn(18, generator=g).cuda().half()
        rows = bev.conv_offset_nhwc(x, wo, bo)                               # [n, 32, H, W] channels-last
        planar = rows[:, :18].contiguous()                                   # the DCNv2 entry's planar offsets
        ones = torch.ones(n, 9, H, W, dtype=torch.float16, device="cuda")

        def one_launch():
            return bev.deform_conv2d_nhwc(x, rows, w, None, groups=G)

        def dcnv2():
            return bev.modulated_deformable_conv2d_nhwc(x, planar, ones, w, None, 1, 1, 1, G, 1)

        def offset_conv():
            return bev.conv_offset_nhwc(x, wo, bo)

        diff = (one_launch().float() - dcnv2().float()).abs().max().item()
        graphs = {"deform_conv": _capture(one_launch)[0], "dcnv2_ones_mask": _capture(dcnv2)[0],
                  "offset_conv": _capture(offset_conv)[0]}
        ms = _alternate(graphs, a)
        recs.append(_record("op", f"deformable 3 x 3, 256 -> 256, groups 4, ({n}, 256, 16, 44), channels-last fp16, "
                            "HIP-graph replay", ms, a, batch=n, max_abs_diff=diff))
    return recs


def _models():
    import torch
    from bevformer_tensorrt_amd import bevdet as D
    models = {"dcn": D.BEVDet(D.BEVDEPTH_R50_DCN, seed=0, bev_half="hip").cuda().half(),
              "no_dcn": D.BEVDet(D.BEVDEPTH_R50, seed=0, bev_half="hip").cuda().half()}
    dcn = models["dcn"].view.depth_net.dcn
    with torch.no_grad():       # live offsets of about a pixel (the zero initialisation samples at the integer taps)
        dcn.conv_offset.bias.copy_(torch.randn(18, generator=torch.Generator().manual_seed(2)).to(dcn.conv_offset.bias))
    calib = models["dcn"].view.calibration_matrices(*D.synthetic_rig(models["dcn"].view)).cuda()
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda().half()
    return models, img, calib


def step_depthnet(a):
    models, img, calib = _models()
    graphs = {}
    for arm, m in models.items():
        m.forward_calibrated(img, calib)                 # (eager: dispatch choices, packed operands)
        x = m.image_features(img.flatten(0, 1))
        mlp = m.view.split_calibration(calib)[1]
        graphs[arm] = _capture(lambda m=m, x=x, mlp=mlp: m.view._depth_feat(x, mlp)[:2])[0]
    ms = _alternate(graphs, a)
    return [_record("depthnet", "BEVDepth DepthNet + softmax / split at R50 (6 x 16 x 44, mid 256, D 59, C 64) on fixed "
                    "image features, with and without the DCN layer, HIP-graph replay, fp16", ms, a)]


def step_frame(a):
    models, img, calib = _models()
    graphs = {}
    for arm, m in models.items():
        m.forward_calibrated(img, calib)
        graphs[arm] = _capture(lambda m=m: m.forward_calibrated(img, calib))[0]
    ms = _alternate(graphs, a)
    return [_record("frame", "BEVDet forward_calibrated, BEVDEPTH_R50_DCN against BEVDEPTH_R50, HIP-graph replay, fp16",
                    ms, a)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "bevdepth_dcn"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bevdepth_dcn_time: needs a GPU (no timing without one)")
        recs = globals()["step_" + a.step](a)
        with open(os.path.join(a.out_dir, a.step + ".jsonl"), "a") as f:
            for r in recs:
                line = json.dumps(r)
                print(line)
                f.write(line + "\n")
        return
    for step, seconds in STEPS:
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step,
               "--alternations", str(a.alternations), "--replays", str(a.replays), "--out-dir", a.out_dir]
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit(f"bevdepth_dcn_time: step {step} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
