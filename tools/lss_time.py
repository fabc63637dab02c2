#!/usr/bin/env python3
"""BEVDet's view-transformer index build on the device (csrc/lss_prepare.hip) timed at BEVDet-R50's shape
(6 x 59 x 16 x 44 frustum points, 128 x 128 x 1 cells), and the whole frame with per-frame calibration.

    python tools/lss_time.py [--rounds 7]        (a) the prepare alone, one JSON line
    python tools/lss_time.py --once              (b) three eager prepares, no timing: for `rocprofv3 --kernel-trace --stats`
    python tools/lss_time.py --frame-ab [--pairs 3]   (c) the whole frame, alternating fresh processes

(a) `us`: functions.lss_voxel_prepare (padded) under HIP-graph replay, median and max over the rounds of one replay of
    `iters` calls each.  The yardstick, `torch_eager_us`, is the torch op sequence of LSSViewTransformer.get_bev_pool_input
    on the same device: its shapes depend on the data and it synchronises the host (boolean-mask selection, argsort,
    torch.where), so it cannot be captured and is timed EAGERLY with a host clock around a synchronise -- what a user
    of the package pays per frame without the kernels.  `host_step_us` is what BEVDetRunner.step adds on the host per
    frame: calibration_matrices + the one upload (host clock, no synchronise inside).
(c) `--frame static`: the static-rank frame the package had before (forward on ranks made beforehand + get_candidates, one
    captured graph; the record tools/decode_time.py --bevdet-frame candidates prints).  `--frame runner`:
    BEVDetRunner(post="candidates") with a FRESH calibration on every frame (jittered_rig(seed = frame)), host work and
    upload included, no synchronise between frames.  Fresh processes alternate; the spread of the static runs is
    printed next to the delta."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bevformer_tensorrt_amd as bev  # noqa: E402,F401
from bevformer_tensorrt_amd import bevdet as D  # noqa: E402
from qkv_time import graph_times_us, stats  # noqa: E402


def host_clock_us(fn, rounds, iters):
    out = []
    for _ in range(2):
        fn()
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / iters)
    return out


def prepare(args):
    dev = torch.device("cuda")
    view = D.LSSViewTransformer(**{k: D.BEVDET_R50[k] for k in ("grid_config", "input_size", "downsample", "in_channels",
                                                                 "out_channels")})
    rig = D.jittered_rig(view, 1)
    calib = view.calibration_matrices(*rig).to(dev)
    ours = lambda: view.prepare_calibrated(calib)
    if args.once:
        for _ in range(3):
            ours()
        torch.cuda.synchronize()
        return
    out = ours()
    n_pts, n_int = out[5].tolist()
    # the yardstick: the reference's op sequence with every tensor on the device
    tview = D.LSSViewTransformer(**{k: D.BEVDET_R50[k] for k in ("grid_config", "input_size", "downsample",
                                                                  "in_channels", "out_channels")})
    tview.frustum = tview.frustum.to(dev)
    drig = [t.to(dev) for t in rig]
    theirs = lambda: tview.get_bev_pool_input(*drig)
    ref = theirs()
    same = all(torch.equal(out[i][:ref[i].numel()], ref[i]) for i in (0, 3, 4)) and ref[0].numel() == n_pts
    staging = torch.zeros(calib.numel(), device=dev)

    def host_step():
        staging.copy_(view.calibration_matrices(*rig))
    rec = {"op": "lss_voxel_prepare", "points": 6 * 59 * 16 * 44, "kept": n_pts, "intervals": n_int,
           "order_free_arrays_equal_torch_on_device": bool(same),
           "us": stats(graph_times_us(ours, 20, args.rounds)),
           "torch_eager_us": stats(host_clock_us(theirs, args.rounds, 10)),
           "ours_eager_us": stats(host_clock_us(ours, args.rounds, 20)),
           "host_step_us": stats(host_clock_us(host_step, args.rounds, 20))}
    rec["speedup_vs_torch_eager"] = round(rec["torch_eager_us"]["median"] / rec["us"]["median"], 1)
    print(json.dumps(rec), flush=True)


def frame(mode, frames=40):
    dev = torch.device("cuda")
    model = D.BEVDet(seed=0).to(dev, torch.float16)
    image = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).to(dev, torch.float16)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if mode == "static":
        ranks = [r.to(dev) for r in model.view.get_bev_pool_input(*D.synthetic_rig(model.view))]
        step = lambda: model.get_candidates(model(image, *ranks), padded=True)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = step()
        for _ in range(5):
            g.replay()
        torch.cuda.synchronize()
        a.record()
        for _ in range(frames):
            g.replay()
        b.record()
        b.synchronize()
        rows = int(out[3][0])
    else:
        runner = D.BEVDetRunner(model, dev, graph=True, post="candidates", clone_outputs=False)
        rigs = [D.jittered_rig(model.view, k) for k in range(frames)]
        out = runner.step(image, *rigs[0])
        image = runner.image_buffer.copy_(image)
        for k in range(5):
            out = runner.step(image, *rigs[k])
        torch.cuda.synchronize()
        a.record()
        for k in range(frames):
            out = runner.step(image, *rigs[k])
        b.record()
        b.synchronize()
        rows = int(out[9][0])
    print(json.dumps({"model": "bevdet_r50", "frame": mode, "postprocess": "candidates", "frames": frames,
                      "ms_per_frame": round(a.elapsed_time(b) / frames, 4), "rows": rows}), flush=True)


def frame_ab(pairs):
    rows = {"static": [], "runner": []}
    for _ in range(pairs):
        for mode in rows:
            cmd = [sys.executable, os.path.abspath(__file__), "--frame", mode]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                raise SystemExit(f"{' '.join(cmd)} failed with {r.returncode}")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rows[mode].append(rec["ms_per_frame"])
            print(json.dumps(rec), flush=True)
    off, on = statistics.median(rows["static"]), statistics.median(rows["runner"])
    print(json.dumps({"frame_ab": "bevdet_r50", "pairs": pairs, "ms_static_ranks": rows["static"],
                      "ms_runner_fresh_calibration": rows["runner"], "median_static": off, "median_runner": on,
                      "static_spread_us": round((max(rows["static"]) - min(rows["static"])) * 1e3, 1),
                      "delta_us": round((on - off) * 1e3, 1), "delta_percent": round((on / off - 1) * 100, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--frame-ab", action="store_true")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--frame", choices=["static", "runner"])
    args = ap.parse_args()
    if args.frame_ab:
        return frame_ab(args.pairs)
    assert torch.cuda.is_available(), "lss_time.py needs the GPU"
    if args.frame:
        return frame(args.frame)
    prepare(args)


if __name__ == "__main__":
    main()
