#!/usr/bin/env python3
"""The LSS depth head (csrc/depth_head.hip) on one MI355X, under HIP-graph replay, arms replayed alternately.

  op      lss_depth_head -- ONE launch -- at (Cin, C, D) = (256, 64, 59) and (256, 64, 88), for 4 224 rows (6 x 16 x 44,
          batch 1) and 33 792 rows (batch 8), channels-last fp16.  D = 59: against dense_auto (the 128-column merged
          depth_net, dispatch by rule) + lss_depth_split, what bev_half="hip" runs there.  D = 88: against the torch
          statements (library 1 x 1 convolution, softmax, the slice / permute copies), what ran there before.
  frame   the captured frame of FLASHOCC_R50_D88 in BEVDetRunner, batch 1: bev_half "hip" against "torch", and
          FLASHOCC_R50 (D = 59) the same way beside it.

Per alternation the mean of `--replays` replays between two events; median and maximum per arm.  One JSON line per
record, appended to profiles/depth_head/<step>.jsonl.  Every step is a child process of its own under `timeout`; the
script stops at the first step that fails.  No ratio here is a gate or a dispatch rule: the records say what was
measured, slower included.

    python tools/depth_head_time.py [--alternations 7] [--replays 20] [--out-dir profiles/depth_head]
    python tools/depth_head_time.py --step op      # one step, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bevdepth_time import _alternate, _capture, _record      # noqa: E402  (the protocol of tools/bevdepth_time.py)

STEPS = (("op", 300), ("frame", 420))      # (name, seconds)


def step_op(a):
    import torch
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd import bevdet as Dm
    Fn = bev.functions
    g = torch.Generator().manual_seed(0)
    Cin, C, recs = 256, 64, []
    for D in (59, 88):
        conv = torch.nn.Conv2d(Cin, D + C, 1).cuda().half()
        packed = Fn.pack_depth_head(conv.weight, conv.bias, D, C)
        for n in (6, 48):
            x = torch.randn(n, 16, 44, Cin, generator=g).cuda().half().permute(0, 3, 1, 2)      # channels-last
            rows = x.permute(0, 2, 3, 1).reshape(-1, Cin)

            def launch():
                return Fn.lss_depth_head(rows, packed, n, spatial=(16, 44))

            if D == 59:
                w, b, lay = Dm.merge_depth_net(conv.weight, conv.bias, D, C)
                other = "dense_auto+lss_depth_split"

                def before():
                    with Dm._rule_dispatch():
                        y = Fn.dense_auto(rows, w, b, None, False)
                    return Fn.lss_depth_split(y, n, D, C, lay["depth_offset"], lay["feat_offset"], spatial=(16, 44))
            else:
                other = "torch_statements"

                def before():
                    with torch.no_grad():
                        y = conv(x)
                    return y[:, :D].softmax(dim=1).contiguous(), y[:, D:D + C].permute(0, 2, 3, 1).contiguous()

            (d0, f0), (d1, f1) = launch(), before()
            diff = max(float((d0.float() - d1.float()).abs().max()), float((f0.float() - f1.float()).abs().max()))
            ms = _alternate({"one_launch": _capture(launch)[0], other: _capture(before)[0]}, a)
            recs.append(_record("op", f"depth head, {rows.shape[0]} rows, Cin {Cin} -> C {C} + D {D}, channels-last fp16, both "
                                f"arms HIP-graph replay; the other arm: {other}", ms, a, rows=rows.shape[0], D=D,
                                max_abs_difference_between_arms=diff))
    return recs


def step_frame(a):
    import torch
    from bevformer_tensorrt_amd import bevdet as D
    dev = torch.device("cuda")
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda().half()
    graphs, runners = {}, []
    for arm, cfg in (("hip", D.FLASHOCC_R50_D88), ("torch", D.FLASHOCC_R50_D88), ("hip_d59", D.FLASHOCC_R50),
                     ("torch_d59", D.FLASHOCC_R50)):
        m = D.BEVDet(cfg, seed=0, bev_half=arm.split("_")[0]).cuda().half()
        runner = D.BEVDetRunner(m, dev, graph=True)
        for _ in range(2):
            runner.step(img, *D.synthetic_rig(m.view))
        torch.cuda.synchronize()
        graphs[arm] = runner._graph
        runners.append(runner)
    ms = _alternate(graphs, a)
    del runners
    return [_record("frame", "the captured frame of FLASHOCC_R50_D88 (index build, image half, depth head, pooling, BEV half, "
                    "occupancy head; post None), 256 x 704, six cameras, fp16, batch 1, in BEVDetRunner, HIP-graph replay: "
                    "bev_half hip against torch; the _d59 arms: FLASHOCC_R50 (D = 59, the two-launch front) the same way, which "
                    "tells the depth head's share from the rest of the BEV half on the 200 x 200 grid", ms, a)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "depth_head"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("depth_head_time: needs a GPU (no timing without one)")
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
            raise SystemExit(f"depth_head_time: step {step} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
