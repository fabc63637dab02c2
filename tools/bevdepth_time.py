#!/usr/bin/env python3
"""BEVDepth's DepthNet on this package's kernels against the plain fp16 path, on one MI355X, under HIP-graph replay.

  depthnet  LSSViewTransformerBEVDepth._depth_feat at R50 (6 x 16 x 44 pixels, mid 256, D 59, C 64) on fixed image
            features: fast (bev_half="hip") and plain fp16 (bev_half="torch") on ONE state dict, replayed alternately;
            per alternation the mean of `--replays` replays between two events; median and maximum per arm
  dilated   the three dilated ASPP layers (256 -> 256, 3 x 3, dilation 6 / 12 / 18, ReLU) on conv_slice_nhwc against
            F.conv2d(dilation=) + bias_act_nhwc_ on channels-last tensors, the same protocol per layer
  frame     BEVDet(BEVDEPTH_R50).forward_calibrated, both arms, the same protocol

One JSON line per record, appended to profiles/bevdepth/<step>.jsonl.  Every step is a child process of its own under
`timeout`; the script stops at the first step that fails.  No ratio here is a gate: the records say what was measured.

    python tools/bevdepth_time.py [--alternations 7] [--replays 20] [--out-dir profiles/bevdepth]
    python tools/bevdepth_time.py --step dilated      # one step, in this process"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("depthnet", 300), ("dilated", 240), ("frame", 420))      # (name, seconds)


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
    """{arm: graph} -> {arm: [ms per alternation]}, arms replayed in turn."""
    for g in graphs.values():
        _replay_ms(g, 5)
    ms = {arm: [] for arm in graphs}
    for _ in range(max(5, a.alternations)):
        for arm, g in graphs.items():
            ms[arm].append(round(_replay_ms(g, a.replays), 4))
    return ms


def _record(step, workload, ms, a, **extra):
    import torch
    rec = {"step": step, "workload": workload, "replays": a.replays, "alternations": len(next(iter(ms.values()))),
           "device": torch.cuda.get_device_name(0)}
    rec.update(extra)
    for arm, v in ms.items():
        rec[f"ms_{arm}"] = v
        rec[f"median_ms_{arm}"] = round(statistics.median(v), 4)
        rec[f"max_ms_{arm}"] = max(v)
    return rec


def _models():
    import torch
    from bevformer_tensorrt_amd import bevdet as D
    fast = D.BEVDet(D.BEVDEPTH_R50, seed=0, bev_half="hip").cuda().half()
    plain = D.BEVDet(D.BEVDEPTH_R50, seed=0, bev_half="torch").cuda().half()
    plain.load_state_dict(fast.state_dict())
    calib = fast.view.calibration_matrices(*D.synthetic_rig(fast.view)).cuda()
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda().half()
    return {"plain": plain, "fast": fast}, img, calib


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
                    "image features, HIP-graph replay, fp16", ms, a)]


def step_dilated(a):
    import torch
    import torch.nn.functional as F
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.functions.yolox_ops import nhwc_empty
    g = torch.Generator().manual_seed(0)
    n, c, H, W = 6, 256, 16, 44
    x = nhwc_empty(n, c, H, W, "cuda")
    x.copy_(torch.randn(n, c, H, W, generator=g).cuda())
    recs = []
    for d in (6, 12, 18):
        w = (torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5).cuda().half()
        wl = w.contiguous(memory_format=torch.channels_last)
        b = torch.randn(c, generator=g).cuda().half()
        out = nhwc_empty(n, c, H, W, "cuda")

        def lib():
            y = F.conv2d(x, wl, None, 1, d, d)
            if not y.is_contiguous(memory_format=torch.channels_last):
                y = y.contiguous(memory_format=torch.channels_last)
            return bev.bias_act_nhwc_(y, b, None, True)

        def hip():
            return bev.conv_slice_nhwc(x, w, b, "relu", out=out, dilation=d)

        ref, got = lib().float(), hip().float()
        err = (ref - got).abs().max().item()
        graphs = {"library": _capture(lib)[0], "conv_slice": _capture(hip)[0]}
        ms = _alternate(graphs, a)
        recs.append(_record("dilated", f"3 x 3 dilation {d}, 256 -> 256, 6 x 16 x 44, bias + ReLU, channels-last fp16, "
                            "HIP-graph replay", ms, a, dilation=d, max_abs_diff=err))
    return recs


def step_frame(a):
    models, img, calib = _models()
    graphs = {}
    for arm, m in models.items():
        m.forward_calibrated(img, calib)
        graphs[arm] = _capture(lambda m=m: m.forward_calibrated(img, calib))[0]
    ms = _alternate(graphs, a)
    return [_record("frame", "BEVDet(BEVDEPTH_R50) forward_calibrated, HIP-graph replay, fp16", ms, a)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "bevdepth"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bevdepth_time: needs a GPU (no timing without one)")
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
            raise SystemExit(f"bevdepth_time: step {step} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
