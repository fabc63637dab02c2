#!/usr/bin/env python3
"""End-to-end frames/s of the re-hosted BEVFormer (random weights, synthetic 6-camera frames),
measured like the reference: device forward of one frame between two stream syncs, H2D excluded,
first and last frame dropped, FPS = 1000 / mean ms (det2trt/utils/tensorrt.py:72-76,
tools/bevformer/evaluate_trt.py:166-168).
usage: model_bench.py [tiny|small|base ...] [--frames N] [--dtype fp16|fp32] [--profile]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bevformer_tensorrt_amd import bevformer as B, geometry as G  # noqa: E402


def run(name, frames, dtype, graph=False, int8=False, clone=True, static_image=False, decode=False):
    dev = torch.device("cuda")
    if int8:    # the PTQ build of bench.py (base only): int8 plugin sites + LinearQ / Conv2dQ dense layers
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import bench
        runner = bench.ModelFrames(dev, "int8", 1, 0, None, None, graph=graph).runner
    else:
        model = B.BEVFormer(name).to(dev, dtype)
        runner = B.FrameRunner(model, dev, dtype, graph=graph, clone_outputs=clone, decode=decode)
    H, W = B.CONFIGS[name]["image"]
    l2i = G.synthetic_lidar2img((H, W)).to(dev)
    g = torch.Generator().manual_seed(0)
    img = torch.randn(1, 6, 3, H, W, generator=g).to(dev, dtype)
    if static_image:      # the caller fills the frame's static input buffer itself (what FrameRunner.step_raw does)
        runner.image_buffer.copy_(img)
        img = runner.image_buffer
    # two untimed frames: the first frame of a scene and the frames after it replay two different graphs, each
    # captured on first use (rounds 1-3 timed the second capture inside frame 2: their per-frame-synchronised
    # figures, e.g. 59.9 frames/s at base in round 3, were inflated by it)
    for i in range(2):
        can = torch.zeros(18)
        can[0], can[-1] = 0.5 * i - 2.0, 0.8 * i - 2.0
        runner.step(img, can, l2i, "scene")
    ts = []
    for i in range(frames):
        can = torch.zeros(18)
        can[0], can[1], can[-2], can[-1] = 0.5 * i, 0.1 * i, 0.01 * i, 0.8 * i
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.step(img, can, l2i, "scene")
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    core = ts[1:-1]
    ms = sum(core) / len(core)
    return dict(model=name, dtype="int8 build" if int8 else str(dtype)[6:], graph=graph, clone_outputs=clone,
                static_image=static_image, frames=frames, ms_per_frame=round(ms, 3),
                fps=round(1000.0 / ms, 2), first_frame_ms=round(ts[0], 1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="*", default=["tiny", "small", "base"])
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--int8", action="store_true", help="the INT8 (PTQ) build of the base model, as bench.py makes it")
    ap.add_argument("--conv-variant", type=int, default=0, help="bevops_conv3x3_c32_set_variant (A/B)")
    ap.add_argument("--mdconv-variant", type=int, default=0, help="bevops_mdconv_set_variant (A/B)")
    ap.add_argument("--msda-variant", type=int, default=0, help="bevops_msda_set_variant before the frames are captured (A/B), e.g. 3015")
    ap.add_argument("--no-clone", action="store_true", help="hand out the graph's output buffers instead of copies")
    ap.add_argument("--decode", action="store_true", help="FrameRunner(decode=True): the detections are decoded inside the frame")
    ap.add_argument("--static-image", action="store_true", help="images already in the frame's static input buffer")
    a = ap.parse_args()
    if a.conv_variant or a.mdconv_variant:
        from bevformer_tensorrt_amd.utils import load_library
        load_library().bevops_conv3x3_c32_set_variant(a.conv_variant)
        load_library().bevops_mdconv_set_variant(a.mdconv_variant)
    if a.msda_variant:
        from bevformer_tensorrt_amd.utils import load_library
        load_library().bevops_msda_set_variant(a.msda_variant)
    dt = torch.float16 if a.dtype == "fp16" else torch.float32
    for m in a.models:
        print(json.dumps(dict(run(m, a.frames, dt, a.graph, a.int8, not a.no_clone, a.static_image, a.decode),
                              mdconv_variant=a.mdconv_variant, msda_variant=a.msda_variant)), flush=True)
