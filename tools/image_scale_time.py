#!/usr/bin/env python3
"""The BEVFormer tiny / small camera front end (csrc/image_scale.hip) timed at the nuScenes geometry: six raw 900 x 1600
uint8 frames -> normalised, rescaled (0.5: 450 x 800, area form; 0.8: 720 x 1280), padded, fp16 [6, 3, 480, 800] /
[6, 3, 736, 1280].

    python tools/image_scale_time.py [--rounds 9]              (a) the call alone, one JSON line per geometry
    python tools/image_scale_time.py --other-forms             (a') the forms (a) leaves out: channels-last output,
                                                                   fp32 input, fp32 output; `us` alone, no yardstick
    python tools/image_scale_time.py --once                    (b) three eager calls per geometry, no timing: for
                                                                   `rocprofv3 --kernel-trace --stats`
    python tools/image_scale_time.py --frame-ab [--pairs 3]    (c) the tiny frame through `step` and through `step_raw`

(a) `us`: functions.image_normalize_resize_pad under HIP-graph replay (`iters` captured calls per replay), median and max
    over the rounds.  The yardstick `torch_us` is the torch op sequence on the same device, also under graph replay:
    uint8 -> float, channel swap, (x - mean) / std in fp32, F.interpolate(bilinear, align_corners=False), F.pad, half.
    The two graphs are replayed ALTERNATELY in the same process, round by round.  `gb_s` = (bytes of the raw frames +
    bytes of the padded output) over `us`: what the call must move, not a counter.  `torch_max_abs_diff` says how far
    that sequence's fp16 result is from ours (it is not the same arithmetic: no area form, another weight rounding).
(c) `--frame prepared`: FrameRunner(graph=True).step on a prepared image in the static buffer.  `--frame raw`: the same
    runner built with raw_size=(900, 1600), step_raw on its raw buffer: the graph starts with the prepare launch.
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
from qkv_time import stats  # noqa: E402

H0, W0, CAMS = 900, 1600, 6


def raw_frames(dev):
    g = torch.Generator().manual_seed(0)
    return torch.randint(0, 256, (CAMS, H0, W0, 3), generator=g, dtype=torch.uint8).to(dev)


def captured(fn, iters):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def pipeline_kwargs(name):
    p = bev.BEVFORMER_IMAGE_PIPELINES[name]
    return dict(scale=p["scale"], mean=p["mean"], std=p["std"], to_rgb=p["to_rgb"], size_divisor=p["size_divisor"])


OTHER_FORMS = (("u8", torch.float16, True), ("f32", torch.float16, False), ("f32", torch.float16, True),
               ("u8", torch.float32, False))       # (input, output type, channels-last); (a) is u8, fp16, planes


def form_name(src, dtype, channels_last):
    return f"{src}->{'f16' if dtype == torch.float16 else 'f32'}:{'nhwc' if channels_last else 'planes'}"


def other_forms(args):
    dev = torch.device("cuda")
    raw = {"u8": raw_frames(dev)}
    raw["f32"] = raw["u8"].float()
    cases = []
    for name in ("tiny", "small"):
        kw = pipeline_kwargs(name)
        for src, dt, cl in OTHER_FORMS:
            out = bev.image_normalize_resize_pad(raw[src], dtype=dt, channels_last=cl, **kw)
            fn = lambda x=raw[src], out=out, cl=cl, kw=kw: bev.image_normalize_resize_pad(x, channels_last=cl, out=out, **kw)
            cases.append((name, form_name(src, dt, cl), captured(fn, 100), fn))   # (fn keeps `out` alive)
    times = [[] for _ in cases]
    for _ in range(args.rounds):                          # round by round over all forms
        for t, (_, _, g, _) in zip(times, cases):
            t.append(replay_us(g, 100))
    for t, (name, form, _, _) in zip(times, cases):
        print(json.dumps({"op": "image_normalize_resize_pad", "pipeline": name, "form": form, "us": stats(t)}), flush=True)


def prepare(args):
    dev = torch.device("cuda")
    raw = raw_frames(dev)
    for name in ("tiny", "small"):
        p, kw = bev.BEVFORMER_IMAGE_PIPELINES[name], pipeline_kwargs(name)
        Hs, Ws = bev.scaled_size(H0, W0, p["scale"])
        Hp, Wp = bev.padded_size(Hs, Ws, p["size_divisor"])
        out = torch.empty((CAMS, 3, Hp, Wp), dtype=torch.float16, device=dev)
        ours = lambda: bev.image_normalize_resize_pad(raw, out=out, **kw)
        if args.once:
            for _ in range(3):
                ours()
            torch.cuda.synchronize()
            continue
        mean = torch.tensor(p["mean"], device=dev).view(1, 3, 1, 1)
        std = torch.tensor(p["std"], device=dev).view(1, 3, 1, 1)

        def theirs():
            x = raw.permute(0, 3, 1, 2).float()
            if p["to_rgb"]:
                x = x.flip(1)
            x = (x - mean) / std
            x = F.interpolate(x, size=(Hs, Ws), mode="bilinear", align_corners=False)
            return F.pad(x, (0, Wp - Ws, 0, Hp - Hs)).half()
        diff = (theirs().float() - ours().float()).abs().max().item()
        iters_ours, iters_torch = 200, 20
        g_ours, g_torch = captured(ours, iters_ours), captured(theirs, iters_torch)
        t_ours, t_torch = [], []
        for _ in range(args.rounds):                      # alternate, so that both see the same machine
            t_ours.append(replay_us(g_ours, iters_ours))
            t_torch.append(replay_us(g_torch, iters_torch))
        moved = raw.numel() + out.numel() * out.element_size()
        rec = {"op": "image_normalize_resize_pad", "pipeline": name, "raw": [CAMS, H0, W0, 3], "resized": [Hs, Ws],
               "out": [CAMS, 3, Hp, Wp], "out_dtype": "fp16 planes", "bytes_read": raw.numel(),
               "bytes_written": out.numel() * out.element_size(), "us": stats(t_ours), "torch_us": stats(t_torch),
               "torch_max_abs_diff": diff}
        rec["gb_s"] = round(moved / rec["us"]["median"] / 1e3, 1)
        rec["speedup_vs_torch"] = round(rec["torch_us"]["median"] / rec["us"]["median"], 2)
        print(json.dumps(rec), flush=True)


def frame(mode, frames=200):
    from bevformer_tensorrt_amd import bevformer as B, geometry as G
    dev = torch.device("cuda")
    model = B.BEVFormer("tiny", seed=0).to(dev, torch.float16)
    raw = raw_frames(dev)
    l2i = G.synthetic_lidar2img((H0, W0))
    can = torch.zeros(18)
    if mode == "raw":
        runner = B.FrameRunner(model, dev, torch.float16, graph=True, clone_outputs=False, raw_size=(H0, W0))
        raw = runner.raw_buffer.copy_(raw)
        step = lambda: runner.step_raw(raw, can, l2i, "scene")
    else:
        runner = B.FrameRunner(model, dev, torch.float16, graph=True, clone_outputs=False)
        image = runner.image_buffer.copy_(bev.image_normalize_resize_pad(raw, **pipeline_kwargs("tiny"))[None])
        scaled = bev.scale_lidar2img(l2i, 0.5)
        step = lambda: runner.step(image, can, scaled, "scene")
    for _ in range(6):                                   # both graphs (first frame of a scene, later frames) and warm-up
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(frames):
        step()
    b.record()
    b.synchronize()
    print(json.dumps({"model": "bevformer_tiny", "frame": mode, "frames": frames,
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
    print(json.dumps({"frame_ab": "bevformer_tiny", "pairs": pairs, "ms_prepared_image": rows["prepared"],
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
    assert torch.cuda.is_available(), "image_scale_time.py needs the GPU"
    if args.frame:
        return frame(args.frame)
    other_forms(args) if args.other_forms else prepare(args)


if __name__ == "__main__":
    main()
