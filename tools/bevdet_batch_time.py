#!/usr/bin/env python3
"""BEVDet-R50 in batches: samples per second of BEVDetRunner(batch=B) under HIP-graph replay, B in {1, 2, 4, 8}.

  frame   the whole frame with post="bboxes" (raw calibration -> kept boxes), per model (fp16 bev_half="hip"; INT8
          build_int8_bevdet(bev_half="int8")) and entry point (`step` from normalised images; `step_raw` from 900 x 1600
          uint8 camera frames).  One runner per B, each captured by its own first call; the arms (the four B) alternate
          in ONE process.  B = 1 is the yardstick: the one-sample path (1-D calibration buffer, the one-sample index
          build), which batching does not change.  samples/s = B / (median ms per replay).
  halves  where the time goes per B: the image half (`image_features` on B * 6 images) and the BEV half
          (`bev_half_calibrated`) of both models, each as its own graph.
  parts   the index build alone (lss_voxel_prepare at B = 1, lss_voxel_prepare_batched above) and the pooling alone
          (bev_pool_v2_indirect(batch=B), fp16 and int8) per B, with the time per sample.

Per alternation the mean of `--replays` replays between two events; median and maximum per arm over `--alternations`
(>= 5).  One JSON line per record, appended to <out-dir>/<step>.jsonl.  Every step is a child process of its own under
`timeout`; the script stops at the first step that fails.  No ratio here is a gate.

    python tools/bevdet_batch_time.py [--alternations 7] [--replays 20] [--out-dir profiles/bevdet_batch]
    python tools/bevdet_batch_time.py --step parts      # one step, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from yolox_time import _alternate, _capture, _summary   # noqa: E402

STEPS = (("frame", 540), ("halves", 300), ("parts", 240))      # (name, seconds)
BATCHES = (1, 2, 4, 8)
RAW = (900, 1600)


def _models():
    """{"fp16_hip": BEVDet(bev_half="hip"), "int8_bev": build_int8_bevdet(bev_half="int8")} on one state dict"""
    import torch
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.bevdet import BEVDet, synthetic_rig
    fp = BEVDet(seed=0, bev_half="hip").cuda().half()
    ranks = [r.cuda() for r in fp.view.get_bev_pool_input(*synthetic_rig(fp.view))]
    frame = (torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda().half(), *ranks)
    q, _, _ = Q.build_int8_bevdet(fp, torch.device("cuda"), [frame], calibrator="minmax", bev_half="int8")
    return {"fp16_hip": fp, "int8_bev": q}


def _rigs(view, B):
    """the six tensors of B different jittered rigs, leading B (ego2global None)"""
    import torch
    from bevformer_tensorrt_amd.bevdet import jittered_rig
    rigs = [jittered_rig(view, k + 1) for k in range(B)]
    return tuple(None if i == 1 else torch.cat([r[i] for r in rigs], 0) for i in range(6))


def _per_sample(rec, arms):
    """samples/s and ms per sample per arm "B<k>", and the ratio of each B to B = 1"""
    for arm in arms:
        b = int(arm[1:])
        rec[f"samples_per_s_{arm}"] = round(b * 1e3 / rec[f"median_ms_{arm}"], 1)
        rec[f"ms_per_sample_{arm}"] = round(rec[f"median_ms_{arm}"] / b, 4)
    for arm in arms:
        rec[f"samples_per_s_{arm}_over_B1"] = round(rec[f"samples_per_s_{arm}"] / rec["samples_per_s_B1"], 3)
    return rec


def step_frame(a):
    import torch
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    models = _models()
    dev = torch.cuda.get_device_name(0)
    gen = torch.Generator().manual_seed(2)
    recs = []
    for name, model in models.items():
        for entry in ("step", "step_raw"):
            # the runners stay alive beside their graphs: a graph reads its runner's static input buffers, and memory
            # released in between is unmapped when the next capture begins (torch.cuda.graph empties the allocator's cache)
            graphs, kept, runners = {}, {}, []
            for B in BATCHES:
                rig = _rigs(model.view, B)
                runner = BEVDetRunner(model, torch.device("cuda"), graph=True, post="bboxes", clone_outputs=False, batch=B,
                                      raw_size=RAW if entry == "step_raw" else None)
                runners.append(runner)
                if entry == "step":
                    out = runner.step(torch.randn(B, 6, 3, 256, 704, generator=gen).cuda().half(), *rig)
                    graphs[f"B{B}"] = runner._graph
                else:
                    raw = torch.randint(0, 256, (B, 6) + RAW + (3,), generator=gen, dtype=torch.uint8).cuda()
                    out = runner.step_raw(raw if B > 1 else raw[0], rig[0], None, rig[2], rig[5])
                    graphs[f"B{B}"] = runner._graph_raw
                torch.cuda.synchronize()
                kept[f"B{B}"] = [int(c) for c in out[9].tolist()]
                assert tuple(out[0].shape) == (B, 2, 128, 128) and tuple(out[9].shape) == (B,)
            ms = _alternate(graphs, a.alternations, a.replays)
            rec = _summary({"step": "frame", "model": name, "entry": entry, "post": "bboxes",
                            "workload": f"BEVDet-R50, B x [6, 3, 256, 704]"
                                        + (" from 900 x 1600 uint8 frames" if entry == "step_raw" else "")
                                        + ", HIP-graph replay, one graph per B", "kept_boxes_per_sample": kept,
                            "replays": a.replays, "device": dev}, ms)
            recs.append(_per_sample(rec, list(graphs)))
            del graphs, runners
            torch.cuda.empty_cache()
    return recs


def step_halves(a):
    import torch
    models = _models()
    dev = torch.cuda.get_device_name(0)
    gen = torch.Generator().manual_seed(3)
    recs = []
    for name, model in models.items():
        view = model.view
        int8 = name == "int8_bev"
        feats = (lambda im: model._features(im)) if int8 else (lambda im: model.image_features(im.flatten(0, 1)))
        img, half, inputs = {}, {}, []      # (inputs: what the graphs read stays alive as long as they do)
        for B in BATCHES:
            image = torch.randn(B, 6, 3, 256, 704, generator=gen).cuda().half()
            x = feats(image).clone()
            if B == 1:
                calib = view.calibration_matrices(*_rigs(view, 1)).cuda()
            else:
                calib = view.calibration_matrices_batched(*_rigs(view, B)).cuda()
            model.bev_half_calibrated(x, calib)
            inputs.append((image, x, calib))
            img[f"B{B}"] = _capture(lambda image=image: feats(image))
            half[f"B{B}"] = _capture(lambda x=x, calib=calib: model.bev_half_calibrated(x, calib))
        for part, graphs in (("image half (image_features)", img), ("BEV half (bev_half_calibrated)", half)):
            ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, a.replays)
            rec = _summary({"step": "halves", "model": name, "part": part, "replays": a.replays, "device": dev}, ms)
            recs.append(_per_sample(rec, list(graphs)))
        del img, half, inputs
        torch.cuda.empty_cache()
    return recs


def step_parts(a):
    import torch
    from bevformer_tensorrt_amd import functions as fn
    from bevformer_tensorrt_amd.bevdet import BEVDET_R50, LSSViewTransformer
    dev = torch.cuda.get_device_name(0)
    view = LSSViewTransformer(**BEVDET_R50)
    frustum = view.frustum.cuda()
    grid = (view.grid_lower_bound, view.grid_interval, view.grid_size)
    gen = torch.Generator().manual_seed(4)
    build, pool16, pool8, counts, inputs = {}, {}, {}, {}, []      # (inputs: kept alive beside the graphs that read them)
    for B in BATCHES:
        arm = f"B{B}"
        if B == 1:
            calib = view.calibration_matrices(*_rigs(view, 1)).cuda()
            prepare, kw = fn.lss_voxel_prepare, {}
        else:
            calib = view.calibration_matrices_batched(*_rigs(view, B)).cuda()
            prepare, kw = fn.lss_voxel_prepare_batched, dict(batch=B)
        build[arm] = _capture(lambda prepare=prepare, calib=calib: prepare(frustum, calib, *grid))
        rb, rd, rf, ist, il, cnt = (t.clone() for t in prepare(frustum, calib, *grid))
        counts[arm] = cnt.tolist()
        depth = torch.rand(B * 6, 59, 16, 44, generator=gen).softmax(1).half().cuda()
        feat = torch.randn(B * 6, 16, 44, 64, generator=gen).half().cuda()
        d8 = torch.randint(0, 127, (B * 6, 59, 16, 44), generator=gen, dtype=torch.int8).cuda()
        f8 = torch.randint(-127, 127, (B * 6, 16, 44, 64), generator=gen, dtype=torch.int8).cuda()
        idx = (rd, rf, rb, ist, il, cnt)
        inputs.append((calib, depth, feat, d8, f8, idx))
        pool16[arm] = _capture(lambda depth=depth, feat=feat, idx=idx, kw=kw: fn.bev_pool_v2_indirect(depth, feat, *idx, 128, 128, **kw))
        pool8[arm] = _capture(lambda d8=d8, f8=f8, idx=idx, kw=kw: fn.bev_pool_v2_indirect(
            d8, f8, *idx, 128, 128, scales=(1 / 127.0, 0.05, 0.11), **kw))
    recs = []
    for part, graphs in (("index build (lss_voxel_prepare / _batched)", build), ("pooling fp16 (bev_pool_v2_indirect)", pool16),
                         ("pooling int8 (bev_pool_v2_indirect)", pool8)):
        ms = _alternate({k: v[0] for k, v in graphs.items()}, a.alternations, a.replays)
        rec = _summary({"step": "parts", "part": part, "points_intervals": counts, "replays": a.replays, "device": dev}, ms)
        recs.append(_per_sample(rec, list(graphs)))
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "bevdet_batch"))
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
        recs = {"frame": step_frame, "halves": step_halves, "parts": step_parts}[a.step](a)
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
