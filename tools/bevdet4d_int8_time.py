#!/usr/bin/env python3
"""INT8 BEVDet4D (csrc/bev_align_s8.hip, quantization.build_int8_bevdet on a temporal model) on one MI355X, under
HIP-graph replay, arms replayed alternately; the protocol of tools/bevdet4d_time.py.

  op      bev_align_stack on int8 maps -- bevops_bev_align_stack_s8 -- against the fp16 launch of this repository
          (bevops_bev_align_stack_f16) on the same shapes, transforms and slots: (1, 128, 128, 80) with T = 1 and T = 8,
          (8, 128, 128, 80) with T = 1.  Each record carries the bytes either launch must move (curr read once, T past
          maps read, T + 1 slices and the kept frame written) and the share of the HBM peak (8 TB/s) they make over its
          median time.
  frame   the captured frame of the INT8 BEVDET4D_R50 in BEVDet4DRunner against the fp16 BEVDET4D_R50 in the same runner
          and against the INT8 BEVDET_R50 in BEVDetRunner: graph replays after three frames of a drive.  Both INT8 models:
          bev_half="int8", min-max calibration on two synthetic frames.

Per alternation the mean of `--replays` replays between two events; median and maximum per arm.  One JSON line per
record, appended to profiles/bevdet4d_int8/<step>.jsonl.  Every step is a child process of its own under `timeout`; the
script stops at the first step that fails.  No ratio here is a gate: the records say what was measured, slower included.

    python tools/bevdet4d_int8_time.py [--alternations 7] [--replays 20] [--out-dir profiles/bevdet4d_int8]
    python tools/bevdet4d_int8_time.py --step op      # one step, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bevdepth_time import _alternate, _capture, _record      # noqa: E402  (the protocol of tools/bevdepth_time.py)
from bevdet4d_time import HBM_PEAK, _rotation                 # noqa: E402

STEPS = (("op", 300), ("frame", 600))      # (name, seconds)


def step_op(a):
    import torch
    import bevformer_tensorrt_amd as bev
    g = torch.Generator().manual_seed(0)
    recs = []
    for B, T in ((1, 1), (1, 8), (8, 1)):
        H = W = 128
        C = 80
        tf = torch.tensor([[_rotation(H, W, 0.02 * (t + 1) + 0.01 * b, 2.5 * (t + 1), -0.4 * (t + 1)) for t in range(T)]
                           for b in range(B)])
        meta = bev.functions.pack_bev_align_meta(tf, list(range(1, T + 1)), [1] * T, 0).cuda()
        graphs, keep = {}, []
        for arm, dtype in (("int8", torch.int8), ("fp16", torch.float16)):
            make = (lambda s: torch.randint(-127, 128, s, generator=g, dtype=torch.int8).cuda()) if dtype == torch.int8 \
                else (lambda s: torch.randn(s, generator=g).cuda().half())
            curr = make((B, H, W, C)).permute(0, 3, 1, 2)                 # channels-last
            hist = make((T + 1, B, H, W, C)).permute(0, 1, 4, 2, 3)
            graph, out = _capture(lambda curr=curr, hist=hist: bev.functions.bev_align_stack(curr, hist, meta, T))
            assert out.dtype == dtype and tuple(out.shape) == (B, (T + 1) * C, H, W)
            graphs[arm] = graph
            keep.append((curr, hist, out))
        ms = _alternate(graphs, a)
        elements = B * H * W * C * (1 + T + (T + 1) + 1)
        rec = _record("op", f"bev_align_stack, ({B}, 128, 128, 80), T {T}, channels-last, the int8 launch against the fp16 "
                      "launch, both HIP-graph replay", ms, a, batch=B, T=T, bytes_moved_int8=elements, bytes_moved_fp16=2 * elements)
        rec["hbm_share_int8"] = round(elements / (rec["median_ms_int8"] * 1e-3) / HBM_PEAK, 4)
        rec["hbm_share_fp16"] = round(2 * elements / (rec["median_ms_fp16"] * 1e-3) / HBM_PEAK, 4)
        rec["int8_over_fp16"] = round(rec["median_ms_int8"] / rec["median_ms_fp16"], 3)
        recs.append(rec)
    return recs


def step_frame(a):
    import torch
    from bevformer_tensorrt_amd import bevdet as D
    from bevformer_tensorrt_amd.quantization import build_int8_bevdet
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(1)
    img = torch.randn(1, 6, 3, 256, 704, generator=gen).cuda().half()

    def int8(m):
        ranks = [r.cuda() for r in m.view.get_bev_pool_input(*D.synthetic_rig(m.view))]
        frames = [(torch.randn(1, 6, 3, 256, 704, generator=gen).cuda().half(), *ranks) for _ in range(2)]
        return build_int8_bevdet(m, dev, frames, "minmax", bev_half="int8")[0]

    graphs, runners = {}, []
    for arm, cfg, cls, build in (("int8_bevdet4d", D.BEVDET4D_R50, D.BEVDet4DRunner, int8),
                                 ("fp16_bevdet4d", D.BEVDET4D_R50, D.BEVDet4DRunner, lambda m: m),
                                 ("int8_bevdet", D.BEVDET_R50, D.BEVDetRunner, int8)):
        m = D.BEVDet(cfg, seed=0, bev_half="hip").cuda().half()
        runner = cls(build(m), dev, graph=True)
        for f in range(3):                                  # a drive: the ring is full and valid when the timing begins
            s2e, e2g, K, pr, pt, bda = D.synthetic_rig(m.view)
            e2g[..., 0, 3] = 2.3 * f
            runner.step(img, s2e, e2g, K, pr, pt, bda)
        torch.cuda.synchronize()
        graphs[arm] = runner._graph
        runners.append(runner)                              # (kept alive)
    ms = _alternate(graphs, a)
    del runners
    rec = _record("frame", "the captured frame (index build, image half, pooling, BEV half, heads; post None), 256 x 704, six "
                  "cameras: INT8 BEVDET4D_R50 (bev_half int8, num_adj 1, pre_process) and fp16 BEVDET4D_R50 (bev_half hip) in "
                  "BEVDet4DRunner, INT8 BEVDET_R50 (bev_half int8) in BEVDetRunner, HIP-graph replay", ms, a)
    rec["int8_4d_over_fp16_4d"] = round(rec["median_ms_int8_bevdet4d"] / rec["median_ms_fp16_bevdet4d"], 3)
    rec["int8_4d_over_int8"] = round(rec["median_ms_int8_bevdet4d"] / rec["median_ms_int8_bevdet"], 3)
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "bevdet4d_int8"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bevdet4d_int8_time: needs a GPU (no timing without one)")
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
            raise SystemExit(f"bevdet4d_int8_time: step {step} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
