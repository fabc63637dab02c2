#!/usr/bin/env python3
"""PTQ calibration on the device (csrc/calibrate.hip) timed; every mode prints JSON lines.

    python tools/calibrate_time.py --sites CONFIG        (a) one calibration frame of the INT8 engine of CONFIG (tiny /
                                                          base) through a recording calibrator: number of sites, the
                                                          largest boundary tensors
    python tools/calibrate_time.py --collect N [N ...]   (b) calib_collect on fp16 ReLU(randn) tensors of N elements
    python tools/calibrate_time.py --threshold S [S ...] (c) calib_threshold over S sites
    python tools/calibrate_time.py --build CONFIG --calibrator NAME [--frames 3]
                                                         (d) wall time of build_int8_engine, one fresh process per call
    python tools/calibrate_time.py --compare CONFIG      (e) the same calibration frames through the host "entropy" and
                                                          the "entropy_device" calibrator at once: per-site scale ratio

(b) `us`: one collect (three launches) under HIP-graph replay, median and max over the rounds of `iters` calls each;
    `gbytes_per_s` counts the tensor twice (the maximum pass and the histogram pass each read it once).  `host_us` is
    the host calibrator's collect on the same device tensor (abs / max / histc / .cpu(), two synchronisations), timed
    eagerly with a host clock around a synchronise: it cannot be captured.
(c) `us`: one search over S states holding histograms of ReLU(randn) batches, graph replay as above; `host_ms_per_site`
    is quantization.entropy_threshold_bin on one of them (host clock, second call).
(d) wall seconds of the whole build (model construction, calibration frames, freeze) and of its parts."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bevformer_tensorrt_amd as bev  # noqa: E402,F401
from bevformer_tensorrt_amd import quantization as Q  # noqa: E402
from bevformer_tensorrt_amd.functions import calib_collect, calib_state_size, calib_threshold  # noqa: E402
from lss_time import host_clock_us  # noqa: E402
from qkv_time import graph_times_us, stats  # noqa: E402


def frames_of(B, G, config, dev, n):
    H, W = B.CONFIGS[config]["image"]
    l2i = G.synthetic_lidar2img((H, W)).to(dev)
    g = torch.Generator().manual_seed(1)
    out = []
    for i in range(n):
        can = torch.zeros(18)
        can[0], can[1], can[-1] = 0.4 * i, -0.1 * i, 1.0 * i
        out.append((torch.randn(1, 6, 3, H, W, generator=g).to(dev, torch.float16), can, l2i))
    return out


class Recorder(Q.DeviceMinMaxCalibrator):
    """Collects like the device calibrators and notes every tensor's size."""

    def __init__(self):
        super().__init__()
        self.seen = {}

    def collect(self, name, tensor):
        self.seen[name] = (int(tensor.numel()), str(tensor.dtype).split(".")[-1], tuple(tensor.shape))
        super().collect(name, tensor)


def sites(config):
    from bevformer_tensorrt_amd import bevformer as B, geometry as G
    dev = torch.device("cuda")
    rec = Recorder()
    Q.build_int8_engine(B, config, dev, frames_of(B, G, config, dev, 1), calibrator=rec)
    top = sorted(rec.seen.items(), key=lambda kv: -kv[1][0])[:5]
    print(json.dumps({"config": config, "sites": len(rec.seen), "elements_per_frame": sum(v[0] for v in rec.seen.values()),
                      "largest": [{"site": k, "numel": v[0], "dtype": v[1], "shape": v[2]} for k, v in top]}), flush=True)


def collect(sizes, rounds):
    g = torch.Generator().manual_seed(0)
    for n in sizes:
        x = torch.relu(torch.randn(n, generator=g)).to("cuda", torch.float16)
        state = torch.zeros(calib_state_size(), dtype=torch.uint8, device="cuda")
        iters = max(2, min(50, int(2e9 / (4 * n))))
        ours = stats(graph_times_us(lambda: calib_collect(x, state), iters, rounds))
        host = Q.EntropyCalibrator()
        theirs = stats(host_clock_us(lambda: host.collect("s", x), rounds, 5))
        print(json.dumps({"op": "calib_collect", "numel": n, "dtype": "float16", "iters": iters, "us": ours,
                          "gbytes_per_s": round(2 * 2 * n / ours["median"] / 1e3, 1), "host_us": theirs,
                          "speedup_vs_host": round(theirs["median"] / ours["median"], 1)}), flush=True)


def threshold(counts, rounds):
    g = torch.Generator().manual_seed(0)
    size = calib_state_size()
    for s in counts:
        states = torch.zeros(s, size, dtype=torch.uint8, device="cuda")
        for i in range(s):
            x = torch.relu(torch.randn(1 << 16, generator=g) * (1.0 + i % 7)).to("cuda", torch.float16)
            calib_collect(x, states[i])
        rec = {"op": "calib_threshold", "sites": s}
        for method in ("entropy", "percentile"):
            rec[method + "_us"] = stats(graph_times_us(lambda: calib_threshold(states, method), 2, rounds))
        hist = states[0, 64:].view(torch.int64).double().cpu()
        Q.entropy_threshold_bin(hist)
        t0 = time.perf_counter()
        Q.entropy_threshold_bin(hist)
        rec["host_ms_per_site"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["host_threads"] = torch.get_num_threads()
        print(json.dumps(rec), flush=True)


class Both(Q.DeviceEntropyCalibrator):
    """Feeds every tensor to the host entropy calibrator as well."""

    def __init__(self):
        super().__init__()
        self.host = Q.EntropyCalibrator()

    def collect(self, name, tensor):
        self.host.collect(name, tensor)
        super().collect(name, tensor)


def compare(config, n_frames):
    from bevformer_tensorrt_amd import bevformer as B, geometry as G
    dev = torch.device("cuda")
    cal = Both()
    Q.build_int8_engine(B, config, dev, frames_of(B, G, config, dev, n_frames), calibrator=cal)
    ours, theirs = cal.scales(), cal.host.scales()
    ratio = sorted((ours[k] / theirs[k], k) for k in ours)
    bins = cal._results()
    host_bins = {k: Q.entropy_threshold_bin(cal.host._stats[k]["hist"]) for k in ours}
    dbin = sorted((abs(bins[k][3] - host_bins[k]), k) for k in ours)
    print(json.dumps({"op": "entropy_device_vs_entropy", "config": config, "frames": n_frames, "sites": len(ours),
                      "equal_scales": sum(1 for r, _ in ratio if r == 1.0),
                      "equal_bins": sum(1 for d, _ in dbin if d == 0),
                      "ratio_min": [round(ratio[0][0], 6), ratio[0][1]], "ratio_max": [round(ratio[-1][0], 6), ratio[-1][1]],
                      "ratio_median": round(ratio[len(ratio) // 2][0], 6),
                      "sites_beyond_1_percent": sum(1 for r, _ in ratio if abs(r - 1) > 0.01),
                      "largest_bin_difference": [dbin[-1][0], dbin[-1][1]]}), flush=True)


def build(config, calibrator, n_frames):
    from bevformer_tensorrt_amd import bevformer as B, geometry as G
    dev = torch.device("cuda")
    fr = frames_of(B, G, config, dev, n_frames)
    torch.cuda.synchronize()
    marks = {}
    cal = Q.get_calibrator(calibrator)()
    freeze = Q.Int8PluginOps.freeze

    def timed_freeze(self):
        torch.cuda.synchronize()
        marks["frames_done"] = time.perf_counter()
        return freeze(self)

    Q.Int8PluginOps.freeze = timed_freeze
    t0 = time.perf_counter()
    model, qops, note = Q.build_int8_engine(B, config, dev, fr, calibrator=cal)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    print(json.dumps({"op": "build_int8_engine", "config": config, "calibrator": calibrator, "frames": n_frames,
                      "sites": len(qops._scales), "wall_s": round(t1 - t0, 2),
                      "model_and_frames_s": round(marks["frames_done"] - t0, 2),
                      "freeze_s": round(t1 - marks["frames_done"], 2), "host_threads": torch.get_num_threads()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites")
    ap.add_argument("--collect", type=int, nargs="+")
    ap.add_argument("--threshold", type=int, nargs="+")
    ap.add_argument("--build")
    ap.add_argument("--compare")
    ap.add_argument("--calibrator", default="entropy_device")
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "calibrate_time.py needs the GPU"
    if args.sites:
        sites(args.sites)
    if args.collect:
        collect(args.collect, args.rounds)
    if args.threshold:
        threshold(args.threshold, args.rounds)
    if args.build:
        build(args.build, args.calibrator, args.frames)
    if args.compare:
        compare(args.compare, args.frames)


if __name__ == "__main__":
    main()
