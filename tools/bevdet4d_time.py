#!/usr/bin/env python3
"""BEVDet4D's temporal alignment and stacking (csrc/bev_align.hip) on one MI355X, under HIP-graph replay, arms replayed
alternately.

  op      bev_align_stack -- ONE launch -- against the torch op sequence on the same device and dtype (the pixel grid
          times the transform, normalisation, one F.grid_sample per past frame, torch.cat, the copy that keeps the
          frame; channels-last fp16 tensors, the transforms read from a device tensor so that the sequence is captured
          too), at (1, 128, 128, 80) with T = 1 and T = 8 and at B = 8 with T = 1.  The record carries the bytes the
          launch must move (curr read once, T past maps read, T + 1 slices and the kept frame written) and the share of
          the HBM peak (8 TB/s) they make over its median time.
  frame   the captured frame of BEVDET4D_R50 in BEVDet4DRunner against BEVDET_R50 in BEVDetRunner (the single-frame
          detector, whose bits this change leaves alone): graph replays of the two runners after three frames of a drive.

Per alternation the mean of `--replays` replays between two events; median and maximum per arm.  One JSON line per
record, appended to profiles/bevdet4d/<step>.jsonl.  Every step is a child process of its own under `timeout`; the
script stops at the first step that fails.  No ratio here is a gate: the records say what was measured, slower included.

    python tools/bevdet4d_time.py [--alternations 7] [--replays 20] [--out-dir profiles/bevdet4d]
    python tools/bevdet4d_time.py --step op      # one step, in this process"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bevdepth_time import _alternate, _capture, _record      # noqa: E402  (the protocol of tools/bevdepth_time.py)

STEPS = (("op", 300), ("frame", 420))      # (name, seconds)
HBM_PEAK = 8.0e12                          # bytes per second


def _rotation(H, W, angle, dx, dy):
    cx, cy = (W - 1) / 2, (H - 1) / 2
    c, s = math.cos(angle), math.sin(angle)
    return [[c, -s, cx - c * cx + s * cy + dx], [s, c, cy - s * cx - c * cy + dy]]


def step_op(a):
    import torch
    import torch.nn.functional as F
    import bevformer_tensorrt_amd as bev
    g = torch.Generator().manual_seed(0)
    recs = []
    for B, T in ((1, 1), (1, 8), (8, 1)):
        H = W = 128
        C = 80
        curr = torch.randn(B, C, H, W, generator=g).cuda().half().contiguous(memory_format=torch.channels_last)
        hist = torch.randn(T + 1, B, H, W, C, generator=g).cuda().half().permute(0, 1, 4, 2, 3)
        tf = torch.tensor([[_rotation(H, W, 0.02 * (t + 1) + 0.01 * b, 2.5 * (t + 1), -0.4 * (t + 1)) for t in range(T)]
                           for b in range(B)])
        slots = list(range(1, T + 1))
        meta = bev.functions.pack_bev_align_meta(tf, slots, [1] * T, 0).cuda()
        tf_dev = tf.cuda()
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        base = torch.stack((xs, ys, torch.ones_like(xs)), -1).view(1, H * W, 3).cuda()
        scale = torch.tensor([2.0 / (W - 1), 2.0 / (H - 1)]).cuda()

        def launch():
            return bev.functions.bev_align_stack(curr, hist, meta, T)

        def torch_ops():
            parts = [curr]
            for t in range(T):
                pos = base.matmul(tf_dev[:, t].transpose(1, 2))                       # [B, H W, 2] source pixels
                grid = (pos * scale - 1.0).view(B, H, W, 2).half()
                parts.append(F.grid_sample(hist[slots[t]], grid, mode="bilinear", padding_mode="zeros", align_corners=True))
            out = torch.cat(parts, 1)
            hist[0].copy_(curr)
            return out

        diff = (launch().float() - torch_ops().float()).abs().max().item()
        graphs = {"one_launch": _capture(launch)[0], "torch_op_sequence": _capture(torch_ops)[0]}
        ms = _alternate(graphs, a)
        moved = B * H * W * C * 2 * (1 + T + (T + 1) + 1)
        rec = _record("op", f"bev_align_stack, ({B}, 128, 128, 80), T {T}, channels-last fp16, both arms HIP-graph replay "
                      "(the torch arm's grid is fp16, as F.grid_sample demands of fp16 features)", ms, a, batch=B, T=T,
                      max_abs_diff_vs_torch_fp16=diff, bytes_moved=moved)
        rec["hbm_share_one_launch"] = round(moved / (rec["median_ms_one_launch"] * 1e-3) / HBM_PEAK, 4)
        recs.append(rec)
    return recs


def step_frame(a):
    import torch
    from bevformer_tensorrt_amd import bevdet as D
    dev = torch.device("cuda")
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda().half()
    graphs = {}
    for arm, cfg, cls in (("bevdet4d", D.BEVDET4D_R50, D.BEVDet4DRunner), ("bevdet", D.BEVDET_R50, D.BEVDetRunner)):
        m = D.BEVDet(cfg, seed=0, bev_half="hip").cuda().half()
        runner = cls(m, dev, graph=True)
        for f in range(3):                                  # a drive: the ring is full and valid when the timing begins
            s2e, e2g, K, pr, pt, bda = D.synthetic_rig(m.view)
            e2g[..., 0, 3] = 2.3 * f
            runner.step(img, s2e, e2g, K, pr, pt, bda)
        torch.cuda.synchronize()
        graphs[arm] = runner._graph
        graphs[arm + "_runner"] = runner                    # (kept alive)
    runners = {k: graphs.pop(k) for k in list(graphs) if k.endswith("_runner")}
    ms = _alternate(graphs, a)
    del runners
    return [_record("frame", "the captured frame (index build, image half, pooling, BEV half, heads; post None), 256 x 704, six "
                    "cameras, fp16, bev_half hip: BEVDET4D_R50 (num_adj 1, pre_process) in BEVDet4DRunner against BEVDET_R50 "
                    "in BEVDetRunner, HIP-graph replay", ms, a)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "bevdet4d"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bevdet4d_time: needs a GPU (no timing without one)")
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
            raise SystemExit(f"bevdet4d_time: step {step} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
