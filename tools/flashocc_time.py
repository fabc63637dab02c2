#!/usr/bin/env python3
"""FlashOcc's occupancy predictor (csrc/occ_head.hip) on one MI355X, under HIP-graph replay, arms replayed alternately.

  op      occ_head_nhwc -- ONE launch -- against the same head as layers this package already had: tile_gemm (256 -> 512),
          torch's Softplus pass, tile_gemm (512 -> 288), torch's arg-max over the [.., 16, 18] view and the cast to
          uint8; at 1 x 40 000 and 8 x 40 000 rows, channels-last fp16.  The record carries the matrix work (2 rows
          (C Hd + Hd Dz Ncls) flop) and its share of the fp16 matrix peak (2.5 PFLOP/s dense) over the launch's median.
  frame   the captured frame of FLASHOCC_R50 in BEVDetRunner (bev_half "hip", post None), batch 1.

Per alternation the mean of `--replays` replays between two events; median and maximum per arm.  One JSON line per
record, appended to profiles/flashocc/<step>.jsonl.  Every step is a child process of its own under `timeout`; the script
stops at the first step that fails.  No ratio here is a gate or a dispatch rule: the records say what was measured,
slower included.

    python tools/flashocc_time.py [--alternations 7] [--replays 20] [--out-dir profiles/flashocc]
    python tools/flashocc_time.py --step op      # one step, in this process"""
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
F16_MATRIX_PEAK = 2.5e15                   # dense fp16 flop per second


def step_op(a):
    import torch
    import torch.nn.functional as F
    import bevformer_tensorrt_amd as bev
    Fn = bev.functions
    g = torch.Generator().manual_seed(0)
    C, Hd, Dz, Ncls = 256, 512, 16, 18
    n = lambda *s: torch.randn(s, generator=g)                                                        # noqa: E731
    W1, b1 = (2.0 * n(Hd, C) / C ** 0.5).cuda().half(), (0.5 * n(Hd)).cuda().half()
    W2, b2 = (n(Dz * Ncls, Hd) / Hd ** 0.5).cuda().half(), (0.5 * n(Dz * Ncls)).cuda().half()
    packed = Fn.pack_occ_head(W1, b1, W2, b2, Dz, Ncls)
    recs = []
    for B in (1, 8):
        y = n(B, 200, 200, C).cuda().half().permute(0, 3, 1, 2)
        rows = y.permute(0, 2, 3, 1).reshape(-1, C)
        occ = torch.empty((B, 200, 200, Dz), dtype=torch.uint8, device="cuda")

        def launch():
            return Fn.occ_head_nhwc(y, packed, out=occ)

        def layers():
            h = F.softplus(Fn.tile_gemm(rows, W1, b1))
            return Fn.tile_gemm(h, W2, b2).view(-1, Dz, Ncls).argmax(-1).to(torch.uint8)

        same = float((launch().view(-1, Dz) == layers()).float().mean())
        graphs = {"one_launch": _capture(launch)[0], "gemm_softplus_gemm_argmax": _capture(layers)[0]}
        ms = _alternate(graphs, a)
        flop = 2.0 * rows.shape[0] * (C * Hd + Hd * Dz * Ncls)
        rec = _record("op", f"occupancy predictor, {B} x 40 000 rows, 256 -> 512 -> 288 (16 x 18), channels-last fp16, both "
                      "arms HIP-graph replay; the layers arm: tile_gemm, torch softplus, tile_gemm, torch argmax + cast", ms, a,
                      batch=B, rows=rows.shape[0], voxels_equal_share=round(same, 5), matrix_flop=flop)
        rec["f16_matrix_peak_share_one_launch"] = round(flop / (rec["median_ms_one_launch"] * 1e-3) / F16_MATRIX_PEAK, 4)
        recs.append(rec)
    return recs


def step_frame(a):
    import torch
    from bevformer_tensorrt_amd import bevdet as D
    dev = torch.device("cuda")
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda().half()
    graphs, runners = {}, []
    for arm, cfg in (("flashocc", D.FLASHOCC_R50), ("bevdet", D.BEVDET_R50)):
        m = D.BEVDet(cfg, seed=0, bev_half="hip").cuda().half()
        runner = D.BEVDetRunner(m, dev, graph=True)
        for _ in range(2):
            runner.step(img, *D.synthetic_rig(m.view))
        torch.cuda.synchronize()
        graphs[arm] = runner._graph
        runners.append(runner)
    ms = _alternate(graphs, a)
    del runners
    return [_record("frame", "the captured frame (index build, image half, pooling, BEV half, head; post None), 256 x 704, six "
                    "cameras, fp16, bev_half hip, batch 1: FLASHOCC_R50 (200 x 200 grid, final_conv + the predictor launch) "
                    "against BEVDET_R50 (128 x 128 grid, CenterPoint heads) in BEVDetRunner, HIP-graph replay: two "
                    "different models, not two ways to one result", ms, a)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "flashocc"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("flashocc_time: needs a GPU (no timing without one)")
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
            raise SystemExit(f"flashocc_time: step {step} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
