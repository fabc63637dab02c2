#!/usr/bin/env python3
"""The 2-D detectors' camera front end (csrc/image_letterbox.hip) timed at the reference's engine shapes: 32 raw
480 x 640 uint8 frames -> YOLOX's fp16 [32, 3, 640, 640] (uint8 fixed-point resize at scale 1, 114 padding) and
CenterNet's fp16 [32, 3, 672, 672] (float32 resize, centred paste at (16, 16), normalisation last).

    python tools/letterbox_time.py [--rounds 9]              (a) the call alone, one JSON line per pipeline
    python tools/letterbox_time.py --other-forms             (a') the forms (a) leaves out: fp16 channels-last and fp32
                                                                 planes; `us` alone, no yardstick
    python tools/letterbox_time.py --once                    (b) three eager calls per pipeline, no timing: for
                                                                 `rocprofv3 --kernel-trace --stats`
    python tools/letterbox_time.py --frame-ab [--pairs 3]    (c) YOLOX-s at batch 1 through `step` and through `step_raw`

(a) `us`: functions.image_letterbox under HIP-graph replay (`iters` captured calls per replay), median and max over the
    rounds.  The yardstick `torch_us` is the torch op sequence on the same device, also under graph replay: uint8 ->
    float, channel swap, F.interpolate(bilinear, align_corners=False), F.pad with the pad value, (x - mean) / std, half.
    The two graphs are replayed ALTERNATELY in the same process, round by round.  `gb_s` = (bytes of the raw frames +
    bytes of the padded output) over `us`: what the call must move, not a counter.  `torch_max_abs_diff` says how far
    that sequence's fp16 result is from ours (it is not the same arithmetic).
(c) `--frame prepared`: YOLOXRunner(graph=True).step on a prepared image in the static buffer.  `--frame raw`: the same
    runner built with raw_size=(480, 640), step_raw on its raw buffer: the graph starts with the letterbox launch.
    Fresh processes alternate; the spread of the prepared runs is printed next to the delta."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bevformer_tensorrt_amd as bev  # noqa: E402
from image_scale_time import captured, form_name, replay_us  # noqa: E402
from qkv_time import stats  # noqa: E402

BATCH, H0, W0 = 32, 480, 640
GEOMETRIES = {"yolox": bev.yolox_test_geometry, "centernet": bev.centernet_test_geometry}


def raw_frames(dev, batch=BATCH):
    g = torch.Generator().manual_seed(0)
    return torch.randint(0, 256, (batch, H0, W0, 3), generator=g, dtype=torch.uint8).to(dev)


def call(args):
    dev = torch.device("cuda")
    raw = raw_frames(dev)
    for name in ("yolox", "centernet"):
        p, geo = bev.DETECT2D_IMAGE_PIPELINES[name], GEOMETRIES[name](H0, W0)
        (Hs, Ws), (Hp, Wp), (oy, ox) = geo["size"], geo["pad_shape"][:2], geo["offset"]
        out = torch.empty((BATCH, 3, Hp, Wp), dtype=torch.float16, device=dev)
        ours = lambda: bev.image_letterbox(raw, geo, p, out=out)
        if args.once:
            for _ in range(3):
                ours()
            torch.cuda.synchronize()
            continue
        mean = torch.tensor(p["mean"], device=dev).view(1, 3, 1, 1)
        std = torch.tensor(p["std"], device=dev).view(1, 3, 1, 1)
        pad = float(p["pad"][0])

        def theirs():
            x = raw.permute(0, 3, 1, 2).float()
            if p["to_rgb"]:
                x = x.flip(1)
            x = F.interpolate(x, size=(Hs, Ws), mode="bilinear", align_corners=False)
            x = F.pad(x, (ox, Wp - Ws - ox, oy, Hp - Hs - oy), value=pad)
            return ((x - mean) / std).half()
        diff = (theirs().float() - ours().float()).abs().max().item()
        iters_ours, iters_torch = 100, 10
        g_ours, g_torch = captured(ours, iters_ours), captured(theirs, iters_torch)
        t_ours, t_torch = [], []
        for _ in range(args.rounds):                      # alternate, so that both see the same machine
            t_ours.append(replay_us(g_ours, iters_ours))
            t_torch.append(replay_us(g_torch, iters_torch))
        moved = raw.numel() + out.numel() * out.element_size()
        rec = {"op": "image_letterbox", "pipeline": name, "arith": p["arith"], "raw": [BATCH, H0, W0, 3],
               "resized": [Hs, Ws], "offset": [oy, ox], "out": [BATCH, 3, Hp, Wp], "out_dtype": "fp16 planes",
               "bytes_read": raw.numel(), "bytes_written": out.numel() * out.element_size(), "us": stats(t_ours),
               "torch_us": stats(t_torch), "torch_max_abs_diff": diff}
        rec["gb_s"] = round(moved / rec["us"]["median"] / 1e3, 1)
        rec["speedup_vs_torch"] = round(rec["torch_us"]["median"] / rec["us"]["median"], 2)
        print(json.dumps(rec), flush=True)


def other_forms(args):
    dev = torch.device("cuda")
    raw = raw_frames(dev)
    cases = []
    for name in ("yolox", "centernet"):
        geo = GEOMETRIES[name](H0, W0)
        for dt, cl in ((torch.float16, True), (torch.float32, False)):
            out = bev.image_letterbox(raw, geo, name, dtype=dt, channels_last=cl)
            fn = lambda geo=geo, name=name, out=out, cl=cl: bev.image_letterbox(raw, geo, name, channels_last=cl, out=out)
            cases.append((name, form_name("u8", dt, cl), captured(fn, 100), fn))   # (fn keeps `out` alive)
    times = [[] for _ in cases]
    for _ in range(args.rounds):
        for t, (_, _, g, _) in zip(times, cases):
            t.append(replay_us(g, 100))
    for t, (name, form, _, _) in zip(times, cases):
        print(json.dumps({"op": "image_letterbox", "pipeline": name, "form": form, "us": stats(t)}), flush=True)


def frame(mode, frames=300):
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_S, YOLOXRunner
    dev = torch.device("cuda")
    model = YOLOX(YOLOX_S, seed=0)
    model.backbone.stem.conv.weight.data.mul_(1.0 / 64)      # the synthetic weights are balanced for a unit-normal image
    model = model.to(dev, torch.float16)
    raw = raw_frames(dev, 1)
    geo = bev.yolox_test_geometry(H0, W0)
    Hp, Wp = geo["pad_shape"][:2]
    if mode == "raw":
        runner = YOLOXRunner(model, 1, Hp, Wp, graph=True, clone_outputs=False, raw_size=(H0, W0))
        raw = runner.raw_buffer.copy_(raw)
        step = lambda: runner.step_raw(raw)
    else:
        runner = YOLOXRunner(model, 1, Hp, Wp, graph=True, clone_outputs=False)
        image = runner.image_buffer.copy_(bev.image_letterbox(raw, geo, "yolox"))
        step = lambda: runner.step(image)
    for _ in range(6):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(frames):
        step()
    b.record()
    b.synchronize()
    print(json.dumps({"model": "yolox_s", "batch": 1, "input": [Hp, Wp], "frame": mode, "frames": frames,
                      "ms_per_frame": round(a.elapsed_time(b) / frames, 4)}), flush=True)


def frame_ab(pairs):
    rows = {"prepared": [], "raw": []}
    for _ in range(pairs):
        for mode in rows:
            cmd = [sys.executable, os.path.abspath(__file__), "--frame", mode]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                raise SystemExit(f"{' '.join(cmd)} failed with {r.returncode}")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rows[mode].append(rec["ms_per_frame"])
            print(json.dumps(rec), flush=True)
    off, on = statistics.median(rows["prepared"]), statistics.median(rows["raw"])
    print(json.dumps({"frame_ab": "yolox_s", "pairs": pairs, "ms_prepared_image": rows["prepared"],
                      "ms_raw_frames": rows["raw"], "median_prepared": off, "median_raw": on,
                      "prepared_spread_us": round((max(rows["prepared"]) - min(rows["prepared"])) * 1e3, 1),
                      "delta_us": round((on - off) * 1e3, 1), "delta_percent": round((on / off - 1) * 100, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--other-forms", action="store_true")
    ap.add_argument("--frame-ab", action="store_true")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--frame", choices=["prepared", "raw"])
    args = ap.parse_args()
    if args.frame_ab:
        return frame_ab(args.pairs)
    assert torch.cuda.is_available(), "letterbox_time.py needs the GPU"
    if args.frame:
        return frame(args.frame)
    other_forms(args) if args.other_forms else call(args)


if __name__ == "__main__":
    main()
