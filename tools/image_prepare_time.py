#!/usr/bin/env python3
"""BEVDet's camera front end (csrc/image_prepare.hip) timed at the R50 geometry: six raw 900 x 1600 uint8 frames ->
PIL-exact resize to 704 x 396, rows 140 .. 395, normalised, fp16 channels-last [6, 3, 256, 704].

    python tools/image_prepare_time.py [--rounds 7]          (a) the prepare call alone, one JSON line
    python tools/image_prepare_time.py --once                (b) three eager calls, no timing: for `rocprofv3 --kernel-trace --stats`
    python tools/image_prepare_time.py --frame-ab [--pairs 3]   (c) the whole frame with / without the prepare launch

(a) `us`: functions.image_resize_crop_normalize under HIP-graph replay, median and max over the rounds of one replay
    of `iters` calls each; `read_gb_s` = the source bytes the crop needs (rows the kept output rows touch, all columns)
    over that time.  The yardstick, `torch_us`, is the same geometry as a torch op sequence on the same device, also
    under graph replay: uint8 -> float -> F.interpolate(bicubic, antialias=True) -> crop -> normalise -> half (time
    only: it is not bit-equal to PIL; `torch_vs_ours_u8` says how far its resized, rounded pixels are from ours).
    `pil_ms_per_image` is PIL on THIS host's CPU when PIL is installed, else null.
(c) `--frame prepared`: BEVDetRunner(post="bboxes").step on a prepared image.  `--frame raw`: the same runner built with
    raw_size=(900, 1600), step_raw: the graph starts with the prepare launch.  Fresh processes alternate; the spread of
    the prepared runs is printed next to the delta."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bevformer_tensorrt_amd as bev  # noqa: E402
from bevformer_tensorrt_amd import bevdet as D  # noqa: E402
from qkv_time import graph_times_us, stats  # noqa: E402

H0, W0, CAMS = 900, 1600, 6


def raw_frames(dev):
    g = torch.Generator().manual_seed(0)
    return torch.randint(0, 256, (CAMS, H0, W0, 3), generator=g, dtype=torch.uint8).to(dev)


def prepare(args):
    dev = torch.device("cuda")
    resize, dims, crop, flip, _ = bev.bevdet_test_augmentation(H0, W0, D.DATA_CONFIG_R50)
    plan = bev.image_resize_plan(H0, W0, dims, crop, dev)
    raw = raw_frames(dev)
    fH, fW = plan.out_size
    out = torch.empty((CAMS, 3, fH, fW), dtype=torch.float16, device=dev, memory_format=torch.channels_last)
    ours = lambda: bev.image_resize_crop_normalize(raw, plan, channels_last=True, out=out)
    if args.once:
        for _ in range(3):
            ours()
        torch.cuda.synchronize()
        return
    by = plan.tables()[2]
    rows = int(by[-1, 0] + by[-1, 1] - by[0, 0])
    read = CAMS * rows * W0 * 3
    mean = torch.tensor(bev.functions.image.BEVDET_IMG_NORM["mean"], device=dev).view(1, 3, 1, 1)
    std = torch.tensor(bev.functions.image.BEVDET_IMG_NORM["std"], device=dev).view(1, 3, 1, 1)

    def resized():
        x = raw.permute(0, 3, 1, 2).float()
        return F.interpolate(x, size=(dims[1], dims[0]), mode="bicubic", antialias=True)[:, :, crop[1]:crop[3], crop[0]:crop[2]]

    def theirs():
        x = resized().flip(1)                                   # to_rgb on an RGB image: the BEVDet channel order
        return ((x - mean) / std).half().contiguous(memory_format=torch.channels_last)
    _, canvas = bev.image_resize_crop_normalize(raw, plan, canvas=True)
    diff = (resized().round().clamp(0, 255) - canvas.permute(0, 3, 1, 2).float()).abs()
    diff = {"max": diff.max().item(), "pixels_differing_percent": round((diff > 0).float().mean().item() * 100, 2)}
    pil_ms = None
    try:
        from PIL import Image
        img = Image.fromarray(raw[0].cpu().numpy())
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            img.resize(dims).crop(crop)
            ts.append((time.perf_counter() - t0) * 1e3)
        pil_ms = round(statistics.median(ts), 2)
    except ImportError:
        pass
    rec = {"op": "image_resize_crop_normalize", "raw": [CAMS, H0, W0, 3], "resize_dims": list(dims), "crop": list(crop),
           "out": "fp16 channels_last", "source_rows_read": rows, "bytes_read": read,
           "us": stats(graph_times_us(ours, 20, args.rounds)),
           "torch_us": stats(graph_times_us(theirs, 5, args.rounds)),
           "torch_vs_ours_u8": diff, "pil_ms_per_image_this_host_cpu": pil_ms}
    rec["read_gb_s"] = round(read / rec["us"]["median"] / 1e3, 1)
    rec["speedup_vs_torch"] = round(rec["torch_us"]["median"] / rec["us"]["median"], 2)
    print(json.dumps(rec), flush=True)


def frame(mode, frames=40):
    dev = torch.device("cuda")
    model = D.BEVDet(seed=0).to(dev, torch.float16)
    s2e, e2g, K, post_rots, post_trans, bda = D.synthetic_rig(model.view)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    raw = raw_frames(dev)
    if mode == "raw":
        runner = D.BEVDetRunner(model, dev, graph=True, post="bboxes", clone_outputs=False, raw_size=(H0, W0))
        runner.step_raw(raw, s2e, e2g, K, bda)
        raw = runner.raw_buffer.copy_(raw)
        step = lambda: runner.step_raw(raw, s2e, e2g, K, bda)
    else:
        runner = D.BEVDetRunner(model, dev, graph=True, post="bboxes", clone_outputs=False)
        resize, dims, crop, flip, _ = bev.bevdet_test_augmentation(H0, W0, D.DATA_CONFIG_R50)
        image = bev.image_resize_crop_normalize(raw, bev.image_resize_plan(H0, W0, dims, crop, dev))[None]
        post_rot, post_tran = bev.bevdet_post_transform(resize, crop, flip)
        post_rots, post_trans = post_rot.view(1, 1, 3, 3).repeat(1, CAMS, 1, 1), post_tran.view(1, 1, 3).repeat(1, CAMS, 1)
        runner.step(image, s2e, e2g, K, post_rots, post_trans, bda)
        image = runner.image_buffer.copy_(image)
        step = lambda: runner.step(image, s2e, e2g, K, post_rots, post_trans, bda)
    for _ in range(5):
        out = step()
    torch.cuda.synchronize()
    a.record()
    for _ in range(frames):
        out = step()
    b.record()
    b.synchronize()
    print(json.dumps({"model": "bevdet_r50", "frame": mode, "postprocess": "bboxes", "frames": frames,
                      "ms_per_frame": round(a.elapsed_time(b) / frames, 4), "boxes": int(out[9][0])}), flush=True)


def frame_ab(pairs):
    rows = {"prepared": [], "raw": []}
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
    off, on = statistics.median(rows["prepared"]), statistics.median(rows["raw"])
    print(json.dumps({"frame_ab": "bevdet_r50", "pairs": pairs, "ms_prepared_image": rows["prepared"],
                      "ms_raw_frames": rows["raw"], "median_prepared": off, "median_raw": on,
                      "prepared_spread_us": round((max(rows["prepared"]) - min(rows["prepared"])) * 1e3, 1),
                      "delta_us": round((on - off) * 1e3, 1), "delta_percent": round((on / off - 1) * 100, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--frame-ab", action="store_true")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--frame", choices=["prepared", "raw"])
    args = ap.parse_args()
    if args.frame_ab:
        return frame_ab(args.pairs)
    assert torch.cuda.is_available(), "image_prepare_time.py needs the GPU"
    if args.frame:
        return frame(args.frame)
    prepare(args)


if __name__ == "__main__":
    main()
