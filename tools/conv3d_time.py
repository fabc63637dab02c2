#!/usr/bin/env python3
"""The 3-D convolution (csrc/conv3d_slice.hip) and BEVDet-Occ's frame on one MI355X, under HIP-graph replay, arms replayed
alternately.

  op      for each distinct layer shape of BEVDET_OCC_R50 (batch 1, a 16 x 200 x 200 volume of 32 channels):
          functions.conv3d_taps -- ONE launch with bias and ReLU in its epilogue -- against F.conv3d on fp16
          channels_last_3d tensors plus the bias / ReLU pass it replaces.  The record carries the matrix work
          (2 M Cout k^3 Cin flop) and its share of the fp16 matrix peak (2.5 PFLOP/s dense) over the launch's median, and
          the largest difference between the arms' outputs.
  frame   the captured frame of BEVDET_OCC_R50 in BEVDetRunner (post None), batch 1: bev_half "hip" against "torch".

Per alternation the mean of `--replays` replays between two events; median and maximum per arm.  One JSON line per
record, appended to profiles/conv3d/<step>.jsonl.  Every step is a child process of its own under `timeout`; the script
stops at the first step that fails.  No ratio here is a gate or a dispatch rule: the records say what was measured,
slower included.

    python tools/conv3d_time.py [--alternations 7] [--replays 20] [--out-dir profiles/conv3d]
    python tools/conv3d_time.py --step op      # one step, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bevdepth_time import _alternate, _capture, _record      # noqa: E402  (the protocol of tools/bevdepth_time.py)

STEPS = (("op", 420), ("frame", 420))      # (name, seconds)
F16_MATRIX_PEAK = 2.5e15                   # dense fp16 flop per second
# (name, Cin, Cout, k, stride, (Z, Y, X), identity) -- every distinct launch shape of the 3-D BEV half
LAYERS = (("stage0 / final_conv 32 -> 32", 32, 32, 3, 1, (16, 200, 200), False),
          ("stage0 conv2 32 -> 32 + identity", 32, 32, 3, 1, (16, 200, 200), True),
          ("stage1 entry 32 -> 64 stride 2", 32, 64, 3, 2, (16, 200, 200), False),
          ("stage1 64 -> 64", 64, 64, 3, 1, (8, 100, 100), True),
          ("stage2 entry 64 -> 128 stride 2", 64, 128, 3, 2, (8, 100, 100), False),
          ("stage2 128 -> 128", 128, 128, 3, 1, (4, 50, 50), True),
          ("LSSFPN3D 1 x 1 x 1 224 -> 32", 224, 32, 1, 1, (16, 200, 200), False))


def step_op(a):
    import torch
    import torch.nn.functional as F
    import bevformer_tensorrt_amd as bev
    Fn = bev.functions
    g = torch.Generator().manual_seed(0)
    recs = []
    for name, cin, cout, k, stride, vol, identity in LAYERS:
        x = torch.randn((1,) + vol + (cin,), generator=g).cuda().half().permute(0, 4, 1, 2, 3)
        w = (torch.randn(cout, cin, k, k, k, generator=g) / (cin * k ** 3) ** 0.5).cuda().half()
        w = w.contiguous(memory_format=torch.channels_last_3d)
        b = (0.5 * torch.randn(cout, generator=g)).cuda().half()
        taps = Fn.conv3d_taps_weight(w)
        out = Fn.conv3d_taps(x, taps, b, "relu", None, stride)
        res = torch.randn(out.permute(0, 2, 3, 4, 1).shape, generator=g).cuda().half().permute(0, 4, 1, 2, 3) if identity else None

        def launch():
            return Fn.conv3d_taps(x, taps, b, "relu", res, stride, out)

        def library():
            y = F.conv3d(x, w, b, stride, k // 2)
            if res is not None:
                y += res
            return y.relu_()

        diff = float((launch().float() - library().float()).abs().max())
        graphs = {"one_launch": _capture(launch)[0], "library_conv3d_bias_relu": _capture(library)[0]}
        ms = _alternate(graphs, a)
        rows = out.numel() // cout
        flop = 2.0 * rows * cout * cin * k ** 3
        rec = _record("op", f"{name}: {cin} -> {cout}, k {k}, stride {stride}, input volume 1 x {vol[0]} x {vol[1]} x {vol[2]}, "
                      f"{'with' if identity else 'no'} identity, bias + ReLU, channels-last fp16, both arms HIP-graph replay",
                      ms, a, rows=rows, max_abs_difference=diff, matrix_flop=flop)
        rec["f16_matrix_peak_share_one_launch"] = round(flop / (rec["median_ms_one_launch"] * 1e-3) / F16_MATRIX_PEAK, 4)
        recs.append(rec)
    return recs


def step_frame(a):
    import torch
    from bevformer_tensorrt_amd import bevdet as D
    dev = torch.device("cuda")
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda().half()
    graphs, runners = {}, []
    for arm in ("hip", "torch"):
        m = D.BEVDet(D.BEVDET_OCC_R50, seed=0, bev_half=arm).cuda().half()
        runner = D.BEVDetRunner(m, dev, graph=True)
        for _ in range(2):
            runner.step(img, *D.synthetic_rig(m.view))
        torch.cuda.synchronize()
        graphs[arm] = runner._graph
        runners.append(runner)
    ms = _alternate(graphs, a)
    del runners
    return [_record("frame", "the captured frame of BEVDET_OCC_R50 (index build, image half, pooling to the 16 x 200 x 200 x 32 "
                    "volume, 3-D BEV half, predictor; post None), 256 x 704, six cameras, fp16, batch 1, in BEVDetRunner, "
                    "HIP-graph replay: bev_half hip against torch", ms, a)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "conv3d"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("conv3d_time: needs a GPU (no timing without one)")
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
            raise SystemExit(f"conv3d_time: step {step} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
