#!/usr/bin/env python3
"""bench.py -- BEVFormer-base frames/s on MI355X (BASELINE.json: "frames/sec BEVFormer-base bs=1 fp16/INT8").

A "step" is ONE MODEL FRAME: six 3x928x1600 camera images -> ResNet-101-DCN + FPN -> 6 encoder layers (temporal
self-attention, spatial cross-attention, FFN over 200x200 BEV queries) -> 6 decoder layers -> heads, through the
reference's stateful frame loop with prev_bev kept on the device (bevformer_tensorrt_amd/bevformer.py: the
mmcv-free re-host of the reference's *TRTP wrappers; random weights and synthetic frames -- no datasets or
checkpoints here).  `value` = frames/s of that step in fp16 (`--dtype int8`: the PTQ engine), replayed from a HIP
graph; every frame carries its own can_bus AND its own calibration matrices (fresh values per frame, as on nuScenes).  N > 1 shards the six cameras over the ranks (backbone, FPN, value projection and the fused SCA sampler on the
local cameras; ONE RCCL all-reduce of the masked camera sums per encoder layer, captured into the graph;
`--exchange gather`: BASELINE config 4's per-camera all-gathers, eager) -- strong scaling: the job is still one frame.

A plain run (`--gpus 1 --steps K --warmup W`) does only what the headline needs: it builds the model, warms up, times
the K frames and prints the line (`value`, `ms_per_step`, `dtype`, ...); the sub-records below are null there.
`--full` measures them too, in the same line (each is still dropped by its --no-* option).  `--dump-outputs DIR` writes
what the timed path handed its caller in the last timed step as DIR/<name>.npy in float32 (end to end: the class
scores and box coordinates of all six decoder layers; --no-end-to-end: the last output of each sampling operator,
as a fixed seeded sample where an output is larger than its share of 60 MB); the inputs are seeded, so the same
arguments give the same inputs on every run and every build.

Sub-records of the same JSON line (N = 1, --full):
  protocol_sync : the reference's own FPS protocol for the same frames (one frame between two stream syncs, first and
                 last dropped, 1000 / mean ms; det2trt/utils/tensorrt.py:72-76) -- also inside every other
                 end-to-end record below;
  int8         : the INT8 counterparts: end_to_end = the PTQ engine (int8 activation chain through the backbone,
                 encoder LinearQ layers, TSA MSDA on the INT8 plugin; quantization.build_int8_engine), hot path, roofline;
  small        : BEVFormer-small fp16 / INT8 end to end (BASELINE config 3);
  bevdet_r50   : BEVDet-R50 fp16 / INT8 end to end (BASELINE config 5);
  hot_path     : one frame's pass over the SAMPLING operators alone at the BEVFormer-base shapes, inputs drawn
                 like the reference's op tests (seed 0; value / offsets / logits ~ N(0,1), reference points
                 ~ U[0,1): the worst case for the sampler; test_multi_scale_deformable_attn.py:25-33):
                     26 DCNv2 convolutions: 23 x (6 cams, 256 ch, 58x100) + 3 x (6 cams, 512 ch, 29x50)
                     rotate(prev_bev [256,200,200])
                     6 x [ TSA MSDA (2, 40000 keys, 40000 q, 1 lvl x 4 pts) + SCA MSDA (6 cams, 30825 keys,
                           40000 q, 4 lvl x 8 pts) ],  6 x decoder MSDA (1, 40000 keys, 900 q, 1 lvl x 4 pts)
  roofline     : achieved algorithmic GB/s of the dominant sampler call (base SCA MSDA, 590.1 MB per call in
                 fp16) from HIP events around every such call of the hot-path step, vs the 8 TB/s
                 HBM peak; .model_geometry / .fused_sca: the same call on the reference points a 6-camera rig
                 produces, as the drop-in op and as the fused SCA op;
  roofline_frame : the SCA sampling call the model frame ACTUALLY replays (fused sampling on the value projection's
                 planes over the balanced slices of a visibility plan + the camera reduce: bevops_sca_forward_planned)
                 on the reference points of the 6-camera rig: its own algorithmic bytes (180.9 MB), HIP-event time,
                 fraction of 8 TB/s -- `roofline` above is the drop-in op on the op test's uniform points;
  roofline_frame_tsa : the TSA sampling call the frame replays (layout-preserving quad kernel on the BEV grid's own
                 reference points; 97.6 MB) the same way;
  frame_calibration : what the per-frame calibration costs inside the frame's graph (camera projection of the BEV
                 pillars, one launch, + the SCA visibility plan, two launches): lidar2img is a per-frame input here as in
                 the reference (tools/bevformer/evaluate_trt.py:99,131-132) and every timed frame gets fresh values;
  roofline_mfma : the frame's largest single kernel, the DCNv2 implicit GEMM of ResNet-101 stage 3 (channels-last
                 entry, 6 x 256 x 58 x 100: 41.05 GFLOP) against the dense fp16 MFMA peak;
  tiny         : BEVFormer-tiny fp16 / INT8 end to end (BASELINE config 2);
  dispatch_misses : dense / convolution problems of this run that the shipped dispatch table does not list (they were
                 measured in-process or defaulted instead);
  cpu_baseline : the sampling operators of a frame on this host's cores through the oracle (kind "port", the base SCA
                 call timed WHOLE), and the whole BEVFormer-tiny in fp32 on the host (BASELINE config 1).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BASE = dict(
    sca=dict(bs=6, levels=[[116, 200], [58, 100], [29, 50], [15, 25]], nq=40000, P=8, ppg=4),
    tsa=dict(bs=2, levels=[[200, 200]], nq=40000, P=4, ppg=1),
    dec=dict(bs=1, levels=[[200, 200]], nq=900, P=4, ppg=1),
    enc_layers=6, dec_layers=6, heads=8, C=32, bev=(200, 200), embed=256,
    # R101-DCN stages 3/4 at 928x1600 (configs/bevformer/bevformer_base.py:42-64): (count, C, H, W)
    dcn=[(23, 256, 58, 100), (3, 512, 29, 50)],
)
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
MFMA_F16_PEAK_TFLOPS = 2500.0  # dense fp16 / bf16 MFMA peak (the task statement's figure; no sparsity)
DUMP_BUDGET_BYTES = 60 * 10 ** 6  # --dump-outputs: values of all files together (under 64 MB with the .npy headers)


def dump_outputs(directory, arrays, budget=DUMP_BUDGET_BYTES):
    """--dump-outputs: every tensor of `arrays` (name -> tensor, None skipped) as directory/<name>.npy in float32.  A
    tensor with more elements than its equal share of `budget` is written as a fixed sample of that many elements:
    flat indices drawn by a generator seeded with 0, in ascending order -- the same elements on every run and every
    build for the same shape.  Returns {name: (shape written, elements of the full tensor)}."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    arrays = {k: v for k, v in arrays.items() if v is not None}
    share = budget // 4 // max(1, len(arrays))
    written = {}
    for name, t in arrays.items():
        t = t.detach()
        if t.numel() > share:
            idx = torch.randint(0, t.numel(), (share,), generator=torch.Generator().manual_seed(0)).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        a = t.float().cpu().numpy()
        np.save(os.path.join(directory, name + ".npy"), a)
        written[name] = (list(a.shape), int(arrays[name].numel()))
    return written


def msda_inputs(cfg, dtype, device, gen, cams=None):
    heads, C = BASE["heads"], BASE["C"]
    L = len(cfg["levels"])
    nk = sum(h * w for h, w in cfg["levels"])
    bs = cfg["bs"] if cams is None else len(cams)
    mk = lambda *s: torch.randn(*s, generator=gen)
    value = mk(cfg["bs"], nk, heads, C)
    ref = torch.rand(cfg["bs"], cfg["nq"], 1, 2 * cfg["ppg"], generator=gen)
    off = mk(cfg["bs"], cfg["nq"], heads, L * cfg["P"] * 2)
    logit = mk(cfg["bs"], cfg["nq"], heads, L * cfg["P"])
    if cams is not None:  # camera shard: same global tensors, local slice
        idx = torch.tensor(cams, dtype=torch.long)
        value, ref, off, logit = (t[idx] if len(cams) else t[:0] for t in (value, ref, off, logit))
    shapes = torch.tensor(cfg["levels"], dtype=torch.int32)
    return [value.to(dtype).to(device), shapes.to(device), ref.to(dtype).to(device),
            off.to(dtype).to(device), logit.to(dtype).to(device)], bs


def msda_bytes(cfg, esize, bs=None):
    heads, C = BASE["heads"], BASE["C"]
    L = len(cfg["levels"])
    nk = sum(h * w for h, w in cfg["levels"])
    bs = cfg["bs"] if bs is None else bs
    n = bs * (nk * heads * C + cfg["nq"] * 2 * cfg["ppg"] + cfg["nq"] * heads * L * cfg["P"] * 3 +
              cfg["nq"] * heads * C)
    return n * esize + 8 * L


def cpu_baseline(max_seconds=30.0):
    """The WHOLE hot-path step on the host cores (port), fp32, on a bounded sample scaled to a frame:
      * MSDA: the reference's PyTorch CPU path (oracle/torch_ref.py) -- one base TSA call, one base
        decoder call and one WHOLE base SCA call (6 x each per frame; the SCA call is not run twice: the
        TSA / decoder calls before it have paged the code in);
      * DCNv2: the C restatement of the reference's im2col + GEMM launcher (oracle/mdconv_ref.c,
        OpenMP) on ONE camera image per ResNet stage (6 images x 23 resp. 3 convolutions per frame);
      * rotate: oracle/sampler_ref.c at 256 x 200 x 200, once per frame.
    Returns frames/s and the per-part seconds."""
    import numpy as np
    import oracle
    from oracle import torch_ref
    gen = torch.Generator().manual_seed(0)
    t_frame = 0.0
    parts = []
    for name, cfg, frac in (("tsa", BASE["tsa"], 1.0), ("dec", BASE["dec"], 1.0),
                            ("sca", BASE["sca"], 1.0)):
        c = dict(cfg)
        c["nq"] = max(1, int(cfg["nq"] * frac))
        args, _ = msda_inputs(c, torch.float32, "cpu", gen)
        args[1] = args[1].long()
        if name != "sca":
            torch_ref.msda(*args)  # warm-up
        t0 = time.perf_counter()
        torch_ref.msda(*args)
        dt = (time.perf_counter() - t0) / frac
        parts.append(f"{name}:{dt:.3f}s")
        t_frame += dt * (BASE["enc_layers"] if name != "dec" else BASE["dec_layers"])
    rng = np.random.default_rng(0)
    for count, C, H, W in BASE["dcn"]:
        x = rng.standard_normal((1, C, H, W), dtype=np.float32)
        off = rng.standard_normal((1, 18, H, W), dtype=np.float32)
        m = rng.random((1, 9, H, W), dtype=np.float32)
        w = rng.standard_normal((C, C, 3, 3), dtype=np.float32) * 0.02
        t0 = time.perf_counter()
        oracle.mdconv(x, off, m, w, np.zeros(C, np.float32), (1, 1), (1, 1), (1, 1), 1, 1)
        dt = (time.perf_counter() - t0) * 6          # six camera images per call
        parts.append(f"dcn{C}:{dt:.3f}s")
        t_frame += dt * count
    img = rng.standard_normal((BASE["embed"],) + BASE["bev"], dtype=np.float32)
    t0 = time.perf_counter()
    oracle.rotate(img, 3.0, (100.0, 100.0), 1)
    dt = time.perf_counter() - t0
    parts.append(f"rotate:{dt:.3f}s")
    t_frame += dt
    return 1.0 / t_frame, " ".join(parts)

def cpu_full_model(frames=2):
    """BASELINE config 1: the WHOLE BEVFormer-tiny (R50 + FPN level, 3 encoder + 6 decoder layers,
    heads) in fp32 on the host cores, bs=1, synthetic 6-camera 480x800 frames -- the reference's
    `*TRT` (non-plugin) wrappers' CPU branch (configs/bevformer/bevformer_tiny_trt.py:3-56): torch
    dense layers + the torch statement of the samplers (oracle/ref_ops.py).  Frame protocol of
    evaluate_pth.py: prev_bev carried, 1 warm-up frame untimed."""
    from bevformer_tensorrt_amd import bevformer as B, geometry as G
    from oracle.ref_ops import RefOps
    model = B.BEVFormer("tiny", ops=RefOps, seed=0)
    runner = B.FrameRunner(model, torch.device("cpu"), torch.float32)
    H, W = B.CONFIGS["tiny"]["image"]
    g = torch.Generator().manual_seed(0)
    l2i = G.synthetic_lidar2img((H, W))
    ts = []
    for i in range(frames + 1):
        img = torch.randn(1, 6, 3, H, W, generator=g)
        can = torch.zeros(18)
        can[0], can[1], can[-2], can[-1] = 0.5 * i, 0.1 * i, 0.01 * i, 0.8 * i
        t0 = time.perf_counter()
        runner.step(img, can, l2i, "scene")
        ts.append(time.perf_counter() - t0)
    core = ts[1:]
    return {"config": "BEVFormer-tiny fp32, whole model, PyTorch CPU path (BASELINE config 1)",
            "frames_per_s": round(len(core) / sum(core), 3), "ms_per_frame": round(sum(core) / len(core) * 1e3, 1),
            "cores": torch.get_num_threads(), "frames": len(core)}


def build_workload(bev, kind, dev, my_cams):
    """The per-frame hot-path operands of one flavour ("fp16" | "fp32" | "int8"), resident in HBM."""
    int8 = kind == "int8"
    dtype = torch.float32 if kind == "fp32" else torch.float16
    gen = torch.Generator().manual_seed(0)
    sca, sca_bs = msda_inputs(BASE["sca"], dtype, dev, gen, cams=my_cams)
    tsa, _ = msda_inputs(BASE["tsa"], dtype, dev, gen)
    dec, _ = msda_inputs(BASE["dec"], dtype, dev, gen)
    prev_bev = torch.randn(BASE["embed"], *BASE["bev"], generator=gen).to(dtype).to(dev)
    rot = (prev_bev, torch.tensor(1.5, device=dev), torch.tensor([100.0, 100.0], device=dev))
    dcn = []
    ncam = len(my_cams)
    for count, C, H, W in BASE["dcn"]:
        if ncam == 0:
            continue
        x = torch.randn(ncam, C, H, W, generator=gen).to(dtype).to(dev)
        off = torch.randn(ncam, 18, H, W, generator=gen).to(dtype).to(dev)
        mask = torch.rand(ncam, 9, H, W, generator=gen).to(dtype).to(dev)
        w = (torch.randn(C, C, 3, 3, generator=gen) / (C * 9) ** 0.5).to(dtype).to(dev)
        b = torch.randn(C, generator=gen).to(dtype).to(dev)
        dcn.append((count, (x, off, mask, w, b, 1, 1, 1, 1, 1)))
    ops = (bev.multi_scale_deformable_attn, bev.modulated_deformable_conv2d, bev.rotate)
    if int8:
        # INT8 flavour of the same step: every plugin-boundary tensor quantised per tensor with the
        # scale the native entropy (KL) calibrator gives for it (quantization.py; the reference
        # gets them from TensorRT's IInt8EntropyCalibrator2, calibrator_trt.py:6-92); reference
        # points stay fp16 (the u8 x255 weight flavour); fp32 DCN bias
        from bevformer_tensorrt_amd.quantization import EntropyCalibrator
        cal = EntropyCalibrator()

        def q(name, t):
            cal.collect(name, t)
            sc = cal.scale(name)
            return cal.quantize(t, sc), sc

        def q_msda(name, a):
            v, sv = q(name + ".value", a[0])
            o, so = q(name + ".offsets", a[3])
            w, sw = q(name + ".weights", a[4])
            return (v, a[1], a[2], o, w, sv, so, sw, 1.0 / 127)   # |out| <= max|value| <= ~ 4 sigma

        sca, tsa, dec = q_msda("sca", sca), q_msda("tsa", tsa), q_msda("dec", dec)
        pq, ps = q("prev_bev", prev_bev)
        rot = (pq, rot[1], rot[2], ps, ps)
        dcn_q = []
        for count, a in dcn:
            x, sx = q("dcn.x", a[0]); o, so = q("dcn.off", a[1]); m, sm = q("dcn.mask", a[2]); w, sw = q("dcn.w", a[3])
            dcn_q.append((count, (x, o, m, w, a[4].float(), sx, so, sm, sw, 4.0 / 127, 1, 1, 1, 1, 1)))
        dcn = dcn_q
        ops = (bev.multi_scale_deformable_attn_int8, bev.modulated_deformable_conv2d_int8, bev.rotate_int8)
    return dict(sca=sca, sca_bs=sca_bs, tsa=tsa, dec=dec, rot=rot, dcn=dcn, ops=ops, dtype=dtype, int8=int8,
                esize=1 if int8 else (2 if dtype == torch.float16 else 4))


def run_hot_path(wl, steps, warmup, dev, dist, exchange, world):
    """W untimed + K timed frames of the hot path, barrier + synchronize on both sides, MAX over
    ranks.  Returns (elapsed seconds, [HIP-event pairs around every base SCA call], {name: the last output of each
    operator in the last timed frame})."""
    op_msda, op_dcn, op_rot = wl["ops"]
    nq, embed = BASE["sca"]["nq"], BASE["embed"]
    sca, tsa, dec, rot, dcn, sca_bs = wl["sca"], wl["tsa"], wl["dec"], wl["rot"], wl["dcn"], wl["sca_bs"]
    out_dtype = torch.int8 if wl["int8"] else wl["dtype"]
    empty = torch.empty((0, nq, BASE["heads"], BASE["C"]), dtype=out_dtype, device=dev)
    sca_events = []
    ex = None
    if world > 1:
        from bevformer_tensorrt_amd.camera_shard import CameraExchange
        ex = CameraExchange(dist, BASE["sca"]["bs"], exchange)

    def sca_call(i=None):
        a = sca if i is None else tuple(t[i:i + 1] if k in (0, 2, 3, 4) else t for k, t in enumerate(sca))
        return op_msda(*a)

    def step(record, keep=None):
        def kept(name, t):    # (the last timed frame only: every other frame drops its outputs as they come)
            if keep is not None:
                keep[name] = t

        for (count, a), stage in zip(dcn, ("dcn_stage3", "dcn_stage4")):
            for _ in range(count):
                kept(stage, op_dcn(*a))
        kept("rotate", op_rot(*rot))
        for _ in range(BASE["enc_layers"]):
            kept("tsa_msda", op_msda(*tsa))
            if record and sca_bs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            if ex is not None and exchange == "gather":
                # camera i's all-gather (RCCL, the process group's stream) overlaps the sampling of camera i + 1
                ex.gather(lambda i: sca_call(i).view(1, nq, embed), (nq, embed), out_dtype, dev)
            else:
                out = sca_call() if sca_bs else empty
                kept("sca_msda", out)
                if ex is not None:   # (int8: partial sums in int32 on every rank, whatever its camera count)
                    acc_dt = torch.int32 if wl["int8"] else out.dtype
                    part = out.view(out.shape[0], nq, embed).sum(0, keepdim=True, dtype=acc_dt) if out.shape[0] else \
                        torch.zeros((1, nq, embed), dtype=acc_dt, device=dev)
                    ex.reduce(part)
            if record and sca_bs:
                e1.record()
                sca_events.append((e0, e1))
        for _ in range(BASE["dec_layers"]):
            kept("dec_msda", op_msda(*dec))

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(warmup):
        step(False)
    fence()
    t0 = time.perf_counter()
    last = {}
    for i in range(steps):
        step(True, last if i == steps - 1 else None)
    fence()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed, sca_events, last


def pmc_traffic(int8):
    """HBM/fabric bytes per base-SCA call from the newest committed rocprofv3 PMC passes
    (FETCH_SIZE and WRITE_SIZE in separate runs; FETCH_SIZE doubled per the gfx950
    correction for 16-byte-per-lane loads, MI355X_MICROARCH.md "HBM").  The call is two
    launches (re-layout, visibility pre-pass, gather); all are summed.  fp16: msda_hm3_repack + msda_hm5_*; int8: msda_hm4_*."""
    try:
        import glob
        f = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "rocprofv3_pmc_fetch_write_per_kernel.json")))[-1]
        total = 0.0
        for k, v in json.load(open(f)).items():
            if int8:
                hit = "msda_hm4_repack_i8" in k or ("msda_hm4_kernel<32" in k and ", true," in k)   # <32, 4 | 6, 512, true, ...>
            else:
                # (msda_hm5_kernel<1>: the drop-in call's sampler behind its visibility pre-pass; <3> is the planned
                # kernel of roofline_frame, <2, 1024, 0, 1 ...> the same kernel's name in the profiles of rounds 3-4)
                hit = ("msda_hm5_kernel<1>" in k or "msda_hm5_kernel<1, false>" in k or "msda_hm5_kernel<2, 1024, 0, 1" in k
                       or "msda_hm5_vis_kernel" in k or "msda_hm3_repack_kernel" in k)
            if hit and "FETCH_SIZE_KiB_avg" in v and "WRITE_SIZE_KiB_avg" in v:
                total += (2 * v["FETCH_SIZE_KiB_avg"] + v["WRITE_SIZE_KiB_avg"]) * 1024
        return (int(total) if total else None), os.path.relpath(f, ROOT)
    except Exception:
        return None, None


def pmc_kernels(pattern, *needles):
    """(bytes, source) of the kernels whose names hold one of `needles` in the newest committed per-kernel PMC file
    matching `pattern` under profiles/r*/ (2 x FETCH_SIZE + WRITE_SIZE: the gfx950 correction), or (None, None)."""
    try:
        import glob
        f = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", pattern)))[-1]
        tot = sum((2 * v["FETCH_SIZE_KiB_avg"] + v["WRITE_SIZE_KiB_avg"]) * 1024 for k, v in json.load(open(f)).items()
                  if isinstance(v, dict) and "FETCH_SIZE_KiB_avg" in v and "WRITE_SIZE_KiB_avg" in v and any(n in k for n in needles))
        return (int(tot), os.path.relpath(f, ROOT)) if tot else (None, None)
    except Exception:
        return None, None


def sca_roofline(wl, sca_events):
    if not sca_events:
        return None
    ms = [a.elapsed_time(b) for a, b in sca_events]
    avg_ms = sum(ms) / len(ms)
    byt = msda_bytes(BASE["sca"], wl["esize"], bs=wl["sca_bs"])
    if wl["int8"]:   # reference points stay fp16 in the INT8 flavour (296.9 MB)
        byt += wl["sca_bs"] * BASE["sca"]["nq"] * 2 * BASE["sca"]["ppg"] * (2 - wl["esize"])
    achieved = byt / (avg_ms * 1e-3) / 1e9
    kern = ("base SCA MSDA call = msda_hm4_repack_i8_kernel + msda_hm4_kernel<32,6,int8 x255 flavour, 2 blocks/CU>" if wl["int8"]
            else "base SCA MSDA call = msda_hm3_repack_kernel + msda_hm5_vis_kernel + msda_hm5_kernel<1>")
    r = {"kernel": kern, "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None, "traffic_src": None,
         "bytes_per_launch": byt, "avg_launch_us": round(avg_ms * 1e3, 2), "launches": len(ms)}
    if wl["sca_bs"] == BASE["sca"]["bs"]:
        r["traffic"], r["traffic_src"] = pmc_traffic(wl["int8"])
    return r


def time_us(fn, iters=10, warm=3):
    for _ in range(warm):
        fn()
    evs = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in evs) / len(evs) * 1e3


def geometry_rooflines(bev, wl, dev):
    """The same SCA call on the reference points the MODEL produces (BEV pillars projected into a
    6-camera rig, geometry.py: 81 % of the (camera, pillar) pairs out of view), as the drop-in op and
    as the fused SCA op (camera-shared offsets / logits read once, invisible pairs skipped, masked
    camera sum inside; SURVEY.md 8d: its own byte count, 282.9 MB)."""
    from bevformer_tensorrt_amd import geometry as G
    img_hw = (928, 1600)
    nq = BASE["sca"]["nq"]
    ref3d = G.reference_points_3d(200, 200, 8, 4, device="cpu")
    cam, mask = G.point_sampling(ref3d, [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], G.synthetic_lidar2img(img_hw), img_hw)
    sca = wl["sca"]
    dtype = wl["dtype"]
    rig = list(sca)
    rig[2] = torch.nan_to_num(cam.reshape(6, nq, 1, 8), nan=-5.0, posinf=5.0, neginf=-5.0).to(dtype).to(dev)
    us = time_us(lambda: bev.multi_scale_deformable_attn(*rig))
    byt = msda_bytes(BASE["sca"], wl["esize"])
    out = {"model_geometry": {"what": "drop-in op, reference points of the 6-camera rig", "bytes_per_launch": byt,
                              "avg_launch_us": round(us, 2), "achieved": round(byt / us / 1e3, 1),
                              "frac": round(byt / us / 1e3 / HBM_PEAK_GBS, 4)}}
    heads, C, LP = BASE["heads"], BASE["C"], 32
    nk = sum(h * w for h, w in BASE["sca"]["levels"])
    fused_bytes = (6 * nk * heads * C + nq * heads * LP * 3 + 6 * nq * 8 + 6 * nq + nq * heads * C) * 2 + 8 * 4
    bm = mask.to(dtype).to(dev)
    us = time_us(lambda: bev.spatial_cross_attention_sample(rig[0], rig[1], rig[2], rig[3][:1], rig[4][:1], bm))
    out["fused_sca"] = {"what": "bevops_sca_forward on the same inputs (SURVEY 8f-3)", "bytes_per_launch": fused_bytes,
                        "avg_launch_us": round(us, 2), "achieved": round(fused_bytes / us / 1e3, 1),
                        "frac": round(fused_bytes / us / 1e3 / HBM_PEAK_GBS, 4)}
    return out


def graph_us(fn, iters=10, rounds=4):
    """Microseconds per call of `fn` under HIP-graph replay -- how the frame launches its kernels: `iters` calls
    captured once, `rounds` + 2 replays, each between two HIP events on the replay's stream; the MEDIAN replay (one
    evidence visit had a single 70 ms stall of the box inside one replay of the DCNv2 record: a mean reported 1 755 us
    for an 80 us call)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    ms = []
    for _ in range(rounds + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); g.replay(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return 0.5 * (ms[(len(ms) - 1) // 2] + ms[len(ms) // 2]) * 1e3 / iters


def frame_rooflines(bev, dev, iters=10, rounds=4):
    """roofline_frame + roofline_mfma (see the module docstring): the two kernels the graph-replayed frame spends its
    sampling time in, each launched as the frame launches it (HIP-graph replay, HIP events around every replay of
    `iters` launches)."""
    from bevformer_tensorrt_amd import geometry as G
    from bevformer_tensorrt_amd.functions import spatial_cross_attention as S
    from bevformer_tensorrt_amd.functions.multi_scale_deformable_attn import _host_shapes, _shapes_i32
    from bevformer_tensorrt_amd.utils import lib as _lib
    out = {}
    g = torch.Generator().manual_seed(0)
    levels = BASE["sca"]["levels"]
    nk = sum(h * w for h, w in levels)
    nq, heads, embed = BASE["sca"]["nq"], BASE["heads"], BASE["embed"]
    try:
        feats = (torch.randn(6, nk, embed, generator=g) * 0.5).half().to(dev)
        wgt = (torch.randn(embed, embed, generator=g) / 16).half().to(dev)
        bias = (torch.randn(embed, generator=g) * 0.1).half().to(dev)
        ref3d = G.reference_points_3d(200, 200, 8, 4, device="cpu")
        cam, mask = G.point_sampling(ref3d, [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], G.synthetic_lidar2img((928, 1600)),
                                     (928, 1600))
        ref = cam.reshape(6, nq, 1, 8).half().to(dev)
        vis = mask.reshape(6, nq, -1).any(-1)
        bm = (vis.float() / vis.sum(0).clamp(min=1)).half().to(dev)
        off = torch.randn(1, nq, heads, 64, generator=g).half().to(dev)
        w = torch.randn(1, nq, heads, 32, generator=g).half().to(dev)
        handle = _lib.load_library()
        shapes_dev, shapes_host = _shapes_i32(torch.tensor(levels, dtype=torch.int32), dev)
        if shapes_host is None:
            shapes_host = _host_shapes(shapes_dev)
        geom = (shapes_host, 6, nk, heads, 32, 4, nq, 8, 4)
        planes = S._project_planes(handle, feats, wgt, bias, geom)
        plan = S.spatial_cross_attention_plan(bm)
        us = graph_us(lambda: S._sample_planes(handle, planes, geom, ref, off, w, bm, plan), iters, rounds)
        byt = (6 * nk * heads * 32 + nq * heads * 32 * 3 + 6 * nq * 8 + 6 * nq + nq * heads * 32) * 2 + 8 * 4
        out["roofline_frame"] = {
            "kernel": "in-frame SCA sampling call = msda_hm5_kernel<3, true> (balanced slices of the visibility plan, pairs only "
                      "one camera sees stored straight into the output) + sca_camera_reduce_kernel<6, true> (the other "
                      "queries), on the value projection's planes",
            "what": "reference points of the 6-camera rig (%.1f %% of the (camera, query) pairs visible), N(0,1) px offsets"
                    % (100.0 * float(vis.float().mean())),
            "bound": "hbm", "bytes_per_launch": byt, "avg_launch_us": round(us, 2), "launches": iters * rounds,
            "timing": "HIP-graph replay", "achieved": round(byt / us / 1e3, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(byt / us / 1e3 / HBM_PEAK_GBS, 4), "traffic": None, "traffic_src": None}
        # fabric bytes of the two kernels from the newest committed PMC passes (not the A/B partners <2, false> / <6, false>)
        out["roofline_frame"]["traffic"], out["roofline_frame"]["traffic_src"] = pmc_kernels(
            "sca_plan_pmc_fetch_write.json", "msda_hm5_kernel<3, true>", "msda_hm5_kernel<3>", "msda_hm5_kernel<2, 1024, 0, 3",
            "sca_camera_reduce_kernel<6, true>")
        del feats, planes
    except Exception as exc:
        out["roofline_frame"] = {"error": repr(exc)[:200]}
    try:   # the frame's TSA sampling call: layout-preserving quad kernel on the BEV grid's own reference points
        cfg = BASE["tsa"]
        ref3d = G.reference_points_3d(200, 200, 8, 4, device="cpu")
        ref2d = G.hybrid_ref_2d(G.reference_points_2d(ref3d), torch.tensor([[0.004, -0.002]]), 1.0).half().to(dev)
        value = torch.randn(2, nq, heads, 32, generator=g).half().to(dev)
        off_t = torch.randn(2, nq, heads, 8, generator=g).half().to(dev)
        w_t = torch.randn(2, nq, heads, 4, generator=g).half().to(dev)
        shp = torch.tensor(cfg["levels"], dtype=torch.int32)
        us = graph_us(lambda: bev.multi_scale_deformable_attn_local(value, shp, ref2d, off_t, w_t), iters, rounds)
        byt = msda_bytes(cfg, 2)
        out["roofline_frame_tsa"] = {
            "kernel": "in-frame TSA sampling call = msda_quad_kernel<__half, 1, 1> (reference layout, no re-layout pass)",
            "what": "reference points of the 200x200 BEV grid with an ego-motion shift (the model's), N(0,1) px offsets",
            "bound": "hbm", "bytes_per_launch": byt, "avg_launch_us": round(us, 2), "launches": iters * rounds,
            "timing": "HIP-graph replay", "achieved": round(byt / us / 1e3, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(byt / us / 1e3 / HBM_PEAK_GBS, 4)}
        # (the hot-path command's TSA launches: same kernel and shapes on the op-test generator's uniform points)
        out["roofline_frame_tsa"]["traffic"], out["roofline_frame_tsa"]["traffic_src"] = pmc_kernels(
            "rocprofv3_pmc_fetch_write_per_kernel.json", "msda_quad_kernel<__half, 1, 1> grid=2560000")
        del value, off_t, w_t
    except Exception as exc:
        out["roofline_frame_tsa"] = {"error": repr(exc)[:200]}
    try:   # what the per-frame calibration costs inside the frame: camera projection of the pillars + plan build
        pillars = G.pillar_points(G.reference_points_3d(200, 200, 8, 4, device="cpu"), [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]).to(dev)
        l2i = G.synthetic_lidar2img((928, 1600)).to(dev)

        def calib():
            _, m = bev.point_sampling(pillars, l2i, (928, 1600), torch.float16)
            S.spatial_cross_attention_plan(m)
        us = graph_us(calib, iters, rounds)
        out["frame_calibration"] = {
            "what": "per-frame calibration work inside the frame's graph: bevops_point_sampling (point_sampling_trt, "
                    "encoder.py:197-259, one launch) + bevops_sca_plan_build (two launches), 6 cameras x 40 000 pillars x 4",
            "avg_us": round(us, 2), "timing": "HIP-graph replay", "launches": iters * rounds}
    except Exception as exc:
        out["frame_calibration"] = {"error": repr(exc)[:200]}
    try:
        B, C, H, W = 6, 256, 58, 100
        x = torch.randn(B, C, H, W, generator=g).half().to(dev).contiguous(memory_format=torch.channels_last)
        om = torch.randn(B, 32, H, W, generator=g).half().to(dev).contiguous(memory_format=torch.channels_last)
        wt = (torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5).half().to(dev)
        bs = torch.randn(C, generator=g).half().to(dev)
        fn = lambda: bev.modulated_deformable_conv2d_nhwc(x, None, None, wt, bs, 1, 1, 1, 1, 1, True, om)  # noqa: E731
        us = graph_us(fn, iters, rounds)
        flop = 2.0 * B * H * W * C * C * 9
        out["roofline_mfma"] = {
            "kernel": "DCNv2 ResNet-101 stage 3, channels-last entry = dcn_glds_f16_kernel<4, 4> (+ dcn_tail_finish_kernel)",
            "bound": "mfma", "flop_per_launch": flop, "avg_launch_us": round(us, 2), "launches": iters * rounds,
            "timing": "HIP-graph replay",
            "achieved": round(flop / us / 1e6, 1), "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(flop / us / 1e6 / MFMA_F16_PEAK_TFLOPS, 4)}
    except Exception as exc:
        out["roofline_mfma"] = {"error": repr(exc)[:200]}
    return out


class ModelFrames:
    """The whole re-hosted BEVFormer-base (backbone, FPN, encoder, decoder, heads; random weights, synthetic
    6-camera frames) behind the reference's stateful frame loop (tools/bevformer/evaluate_trt.py:76-154).
    kind "fp16": fp16 operators; "int8": the PTQ build (quantization.build_int8_engine) -- the backbone as an int8
    ACTIVATION CHAIN (every 1x1 / 3x3 / DCNv2 layer of every bottleneck reads and writes int8, identity rows
    included; det2trt/models/utils/register.py:78-84, configs/bevformer/plugin/bevformer_base_trt_p2_q.py), the
    encoder's dense layers as LinearQ, TSA's MSDA on the INT8 plugin; scales from the native entropy calibrator
    over `calib` synthetic frames; layers whose fp16 form is faster on MI355X (decoder, rotate, SCA's projected
    sampler) stay fp16 -- a mixed engine, as TensorRT builds them.
    N = 1: the frame is replayed from a HIP graph; N > 1: the cameras are sharded (camera_shard.py) and -- with the
    default "reduce" exchange -- the frame is replayed from a HIP graph that holds its RCCL all-reduces too (the
    per-camera all-gather exchange runs eagerly)."""

    def __init__(self, dev, kind, world, rank, dist, exchange, calib=4, graph=True, name="base", sca_int8=False):
        from bevformer_tensorrt_amd import bevformer as B, geometry as G
        self.B, self.dev, self.kind, self.name = B, dev, kind, name
        dtype = torch.float16
        torch.cuda.empty_cache()
        H, W = B.CONFIGS[name]["image"]
        gen = torch.Generator().manual_seed(0)
        self.img = torch.randn(1, 6, 3, H, W, generator=gen).to(dev, dtype)
        # the calibration is a per-FRAME input, as on nuScenes (ego motion between the camera and lidar timestamps; the
        # reference feeds lidar2img to the engine on every frame, tools/bevformer/evaluate_trt.py:99,131-132): every step
        # hands the runner a FRESH host tensor with other values (the rig, jittered), and the frame's graph evaluates the
        # camera projection of the BEV pillars and the SCA visibility plan from it on every replay
        base_l2i = G.synthetic_lidar2img((H, W))
        self.l2is = []
        for k in range(16):
            m = base_l2i.clone()
            m[:, :, :3, 3] += 0.03 * torch.randn(1, 6, 3, generator=gen)          # translation jitter (image-plane units)
            m[:, :, :3, :3] *= 1 + 1e-3 * torch.randn(1, 6, 3, 3, generator=gen)   # rotation / intrinsics jitter
            self.l2is.append(m)
        self.l2i = base_l2i.to(dev)     # (calibration frames of the INT8 build)
        cams = gather = None
        if world > 1 or dist is not None:     # (dist at world 1: the sharded code path on a one-rank group, --sharded-path)
            from bevformer_tensorrt_amd.camera_shard import CameraExchange
            gather = CameraExchange(dist, 6, exchange)
            cams = gather.cams
        self.note = None
        if kind == "int8":
            from bevformer_tensorrt_amd.quantization import build_int8_engine
            frames = [(self.img, self.can(i), self.l2i) for i in range(calib)]
            model, _, self.note = build_int8_engine(B, name, dev, frames, "entropy",
                                                    chain=os.environ.get("BEVOPS_INT8_CHAIN", "1") != "0",
                                                    sca_int8=sca_int8)
        else:
            model = B.BEVFormer(name, seed=0).to(dev, dtype)
        # N > 1: the "reduce" exchange (fused sampler on the local cameras, ONE all-reduce per encoder layer) is
        # captured with its RCCL collectives; the per-camera pipelined all-gathers run eagerly
        self.graph = graph and (gather is None or exchange in ("reduce", "scatter"))
        self._shard = (cams, gather)
        # the graph's own output buffers are handed out (no per-frame clones), and the synthetic camera images sit in
        # the frame's static input buffer, where a serving caller's normalise pass (FrameRunner.step_raw) writes them
        self.runner = B.FrameRunner(model, dev, dtype, cams=cams, gather=gather, graph=self.graph, clone_outputs=False)
        self.runner.image_buffer.copy_(self.img)
        self.img = self.runner.image_buffer
        self.i = 0
        # priming, part of the build and outside every timed region whatever --warmup says: the first frame of a
        # scene and the frames after it replay two different graphs (each captured on first use, after the measured
        # choice of dense-layer / convolution kernels has been made in the capture's warm-up forwards)
        for _ in range(2):
            self.step()

    @staticmethod
    def can(i):
        c = torch.zeros(18)
        c[0], c[1], c[-2], c[-1] = 0.5 * i, 0.1 * i, 0.01 * i, 0.8 * i
        return c

    def step(self):
        self.i += 1
        l2i = self.l2is[self.i % len(self.l2is)].clone()     # a fresh tensor with this frame's values
        try:
            return self.runner.step(self.img, self.can(self.i), l2i, "scene")
        except Exception:
            if not self.graph or self.runner._graph is not None:
                raise
            # graph capture refused (an operator that synchronises during capture): eager frames
            self.graph = False
            img = self.img.clone()
            self.runner = self.B.FrameRunner(self.runner.model, self.dev, torch.float16, cams=self._shard[0],
                                             gather=self._shard[1], clone_outputs=False)
            self.runner.image_buffer.copy_(img)
            self.img = self.runner.image_buffer
            return self.runner.step(self.img, self.can(self.i), l2i, "scene")


def run_frames(frames, steps, warmup, dev, dist):
    """W untimed + K timed model frames, barrier + synchronize on both sides, MAX over ranks.  Returns (elapsed
    seconds, what the last timed frame's `step` returned)."""
    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(warmup):
        frames.step()
    fence()
    t0 = time.perf_counter()
    out = None
    for _ in range(steps):
        out = frames.step()
    fence()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed, out


def run_frames_protocol(frames, steps):
    """The reference's own FPS protocol (det2trt/utils/tensorrt.py:72-76, tools/bevformer/evaluate_trt.py:166-168):
    the device forward of ONE frame between two stream synchronisations, first and last frame dropped,
    FPS = 1000 / mean ms.  (`value` of the line is back-to-back throughput, as bench.py's contract defines a step;
    this is the latency-style figure next to it.)"""
    ts = []
    for _ in range(steps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames.step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    core = ts[1:-1]
    ms = sum(core) / len(core)
    return {"value": round(1000.0 / ms, 3), "unit": "frames/s", "ms_per_frame": round(ms, 4), "frames": len(core),
            "protocol": "per-frame stream sync, first and last frame dropped, 1000 / mean ms (tensorrt.py:72-76)"}


def bevdet_frames(dev, steps, warmup, int8=True):
    """BASELINE config 5: the whole BEVDet-R50 (6 x 3x256x704 -> R50 + FPN -> depth_net -> bev_pool_v2 -> bev encoder ->
    CenterHead; det2trt/models/detector/bevdet.py:29-82), random weights, synthetic rig, HIP-graph replay: fp16, and
    the PTQ build (int8 activation chain through the backbone, INT8 bev_pool_v2); back-to-back frames/s and the
    reference's per-frame-synchronised protocol for each."""
    from bevformer_tensorrt_amd import bevdet as D

    def graphed(model, img, ranks):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                model(img, *ranks)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            model(img, *ranks)

        class _F:
            step = staticmethod(graph.replay)

        el, _ = run_frames(_F, steps, warmup, dev, None)
        return {"value": round(steps / el, 3), "unit": "frames/s", "ms_per_step": round(el / steps * 1e3, 4),
                "hip_graph": True, "protocol_sync": run_frames_protocol(_F, steps)}

    model = D.BEVDet(seed=0).to(dev, torch.float16)
    ranks = [r.to(dev) for r in model.view.get_bev_pool_input(*D.synthetic_rig(model.view))]
    gen = torch.Generator().manual_seed(0)
    hw = D.view_input_size(model.view)
    img = torch.randn(1, 6, 3, *hw, generator=gen).to(dev, torch.float16)
    out = {"config": "BEVDet-R50: 6x(3x256x704) -> ResNet-50 + FPN -> depth_net -> bev_pool_v2 (%d points, %d intervals) "
                     "-> bev encoder + FPN_LSS -> CenterHead" % (ranks[0].numel(), ranks[3].numel()),
           "fp16": graphed(model, img, ranks)}
    del model
    if int8:
        try:
            from bevformer_tensorrt_amd.quantization import build_int8_bevdet
            cal = [(torch.randn(1, 6, 3, *hw, generator=gen).to(dev, torch.float16), *ranks) for _ in range(4)]
            m8, _, note = build_int8_bevdet(D, dev, cal)
            out["int8"] = dict(graphed(m8, img, ranks), build=note)
        except Exception as exc:
            out["int8"] = {"error": repr(exc)[:300]}
    return out


def dispatch_misses():
    """Dense / convolution problems this process posed that bevformer_tensorrt_amd/dispatch_gfx950.json does not list
    (each was measured in-process, or defaulted under capture): the run-to-run kernel choice is only pinned for listed
    problems."""
    try:
        from bevformer_tensorrt_amd.functions import conv as C, linear as L
        return {"dense": list(L.DENSE_MISSES), "conv": list(C.CONV_MISSES)}
    except Exception as exc:
        return {"error": repr(exc)[:120]}


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: spawn the N ranks here (one process per GPU,
    RCCL rendezvous on 127.0.0.1) -- the driver's torch.distributed.run launch sets WORLD_SIZE itself
    and never comes through this path."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable] + sys.argv, env=env))
    rc = 0
    for p in procs:
        rc = rc or p.wait()
    raise SystemExit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "int8"],
                    help="which build of the model the headline `value` times (the other one is a sub-record at N=1)")
    ap.add_argument("--exchange", default="scatter", choices=["gather", "reduce", "scatter"],
                    help="N>1: scatter (default) = cameras sharded and the rest of the encoder sharded by query range: the "
                         "fused sampler on the local cameras, per encoder layer one all-gather of the query rows and one "
                         "reduce-scatter of the masked camera sums (the bytes of one all-reduce), TSA / norms / FFN on a "
                         "rank's own rows, HIP graph with the RCCL collectives inside; reduce = "
                         "all-reduce of each rank's masked camera sum (the fused sampler runs on the local "
                         "cameras, one 20.5 MB collective per encoder layer, the frame replays from a HIP graph with its "
                         "RCCL collectives inside) or the per-camera pipelined all-gathers of the camera features "
                         "(BASELINE config 4's exchange: 6x the data, eager frames)")
    ap.add_argument("--sharded-path", action="store_true",
                    help="run the N > 1 code path (process group, camera / query sharding, collectives inside the frame's "
                         "HIP graph) even with ONE rank: what the GPU test of this file's multi-GPU path uses on a 1-GPU box")
    ap.add_argument("--full", action="store_true",
                    help="also measure the sub-records (INT8 engine, tiny / small / BEVDet, hot path, rooflines, "
                         "reference FPS protocol, CPU baselines); a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy "
                         "(float32, 64 MB at most)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-end-to-end", action="store_true",
                    help="profiling runs: time the sampling hot path only (the line's value is then the hot-path rate)")
    ap.add_argument("--no-int8", action="store_true", help="skip the INT8 sub-records of the default fp16 run")
    ap.add_argument("--no-hot-path", action="store_true", help="skip the hot-path / roofline sub-records")
    ap.add_argument("--int8-sca-plugin", action="store_true",
                    help="also time the INT8 engine with the SCA site on the INT8 plugin (int8.end_to_end_sca_on_int8_plugin)")
    ap.add_argument("--no-small", action="store_true", help="skip the BEVFormer-small end-to-end sub-record")
    ap.add_argument("--no-geometry-extra", action="store_true",
                    help="skip the extra SCA timings on the model's own reference points (profiling runs: keeps "
                         "the rocprofv3 per-kernel averages to the contract workload)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    sharded = world > 1 or args.sharded_path
    if sharded:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:
            os.environ.setdefault("MASTER_PORT", "29571"); os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("nccl", device_id=dev)

    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.camera_shard import camera_shards

    # ---- headline: end-to-end model frames (BASELINE.json: frames/sec BEVFormer-base bs=1 fp16/INT8)
    headline = None
    if not args.no_end_to_end:
        frames = ModelFrames(dev, args.dtype, world, rank, dist, args.exchange)
        elapsed, (cls, crd) = run_frames(frames, args.steps, args.warmup, dev, dist)
        if args.dump_outputs and rank == 0:   # (before anything else replays the frame's graph into these buffers)
            dump_outputs(args.dump_outputs, {"cls_scores": cls, "bbox_preds": crd})
        del cls, crd
        headline = {"elapsed": elapsed, "hip_graph": frames.graph, "note": frames.note, "protocol_sync": None}
        if args.full and not sharded:
            headline["protocol_sync"] = run_frames_protocol(frames, args.steps)
        del frames
        torch.cuda.empty_cache()

    # ---- sub-records (--full: N = 1 and the hot-path step; at N > 1 the hot path is measured when asked to stand
    # alone) -- with --no-end-to-end the hot path is the headline and runs in a plain run too
    my_cams = camera_shards(BASE["sca"]["bs"], world)[rank]
    hot = roofline = None
    if not args.no_hot_path and (not sharded or args.no_end_to_end) and (args.full or headline is None):
        kind = "int8" if args.dtype == "int8" else "fp16"
        wl = build_workload(bev, kind, dev, my_cams)
        el, sca_events, last = run_hot_path(wl, args.steps, args.warmup, dev, dist, args.exchange, world)
        if args.dump_outputs and rank == 0 and headline is None:
            dump_outputs(args.dump_outputs, last)
        del last
        roofline = sca_roofline(wl, sca_events)
        hot = {"what": "one frame's pass over the sampling operators only: 26x DCNv2 + rotate + 6x(TSA + SCA) MSDA "
                       "+ 6x decoder MSDA, op-test inputs (uniform-random reference points)",
               "value": round(args.steps / el, 3), "unit": "frames/s", "ms_per_step": round(el / args.steps * 1e3, 4),
               "steps": args.steps, "warmup": args.warmup, "dtype": "i8" if kind == "int8" else "f16"}
        if roofline is not None and sharded:
            roofline["note"] = ("N>1: rank 0's cameras only (bytes_per_launch counts them); the bracket spans the "
                                "per-camera sampler calls of one encoder layer and the wait for its exchange")
        if roofline is not None and not sharded and kind == "fp16" and not args.no_geometry_extra and args.full:
            try:
                roofline.update(geometry_rooflines(bev, wl, dev))
            except Exception as exc:  # the contract line must still be printed
                roofline["model_geometry"] = {"error": repr(exc)[:160]}
        del wl

    # the other precision, measured in the SAME default run (the metric is "fp16/INT8")
    other = None
    if args.full and not sharded and not args.no_int8 and args.dtype == "fp16":
        other = {"dtype": "i8"}
        if not args.no_hot_path:
            try:
                wl8 = build_workload(bev, "int8", dev, my_cams)
                el8, ev8, _ = run_hot_path(wl8, args.steps, args.warmup, dev, None, args.exchange, 1)
                other["hot_path"] = {"value": round(args.steps / el8, 3), "unit": "frames/s",
                                     "ms_per_step": round(el8 / args.steps * 1e3, 4),
                                     "scales": "entropy (KL) calibrator per plugin-boundary tensor; fp16 reference points "
                                               "(the reference's <__half2> x255-weight flavour); fp32 DCN bias"}
                other["roofline"] = sca_roofline(wl8, ev8)
                del wl8
            except Exception as exc:
                other["hot_path"] = {"error": repr(exc)[:200]}
        if not args.no_end_to_end:
            try:
                f8 = ModelFrames(dev, "int8", 1, 0, None, args.exchange)
                e8, _ = run_frames(f8, args.steps, args.warmup, dev, None)
                other["end_to_end"] = {"value": round(args.steps / e8, 3), "unit": "frames/s",
                                       "ms_per_step": round(e8 / args.steps * 1e3, 4), "hip_graph": f8.graph,
                                       "build": f8.note, "protocol_sync": run_frames_protocol(f8, args.steps)}
                del f8
                torch.cuda.empty_cache()
            except Exception as exc:
                other["end_to_end"] = {"error": repr(exc)[:300]}
            try:   # the same engine with the SCA site on the INT8 plugin too (the reference's INT8 configs' choice): on request
                # only -- design/msda.md (round 6) closes that variant with its instruction budget (1.24-1.30 x the fp16
                # planned sampler's instructions per item in the plugin's arithmetic)
                if not args.int8_sca_plugin:
                    raise StopIteration
                f8 = ModelFrames(dev, "int8", 1, 0, None, args.exchange, sca_int8=True)
                e8, _ = run_frames(f8, args.steps, args.warmup, dev, None)
                other["end_to_end_sca_on_int8_plugin"] = {"value": round(args.steps / e8, 3), "unit": "frames/s",
                                                          "ms_per_step": round(e8 / args.steps * 1e3, 4),
                                                          "hip_graph": f8.graph, "build": f8.note}
                del f8
                torch.cuda.empty_cache()
            except StopIteration:
                pass
            except Exception as exc:
                other["end_to_end_sca_on_int8_plugin"] = {"error": repr(exc)[:300]}

    # BASELINE config 3: BEVFormer-small fp16 / INT8 end to end (same protocol pair)
    small = tiny = None
    if args.full and not sharded and not args.no_end_to_end and not args.no_small:
        small = {"config": "BEVFormer-small: 6x(3x736x1280) -> ResNet-101-DCN (C5) + FPN level -> 3 encoder layers "
                           "(150x150 BEV queries) -> 6 decoder layers -> heads"}
        tiny = {"config": "BEVFormer-tiny (BASELINE config 2): 6x(3x480x800) -> ResNet-50 (C5) + FPN level -> 3 encoder "
                          "layers (50x50 BEV queries) -> 6 decoder layers -> heads; custom MSDA / rotate HIP kernels"}
        for name, rec in (("small", small), ("tiny", tiny)):
            for kind in ("fp16",) + (() if args.no_int8 else ("int8",)):
                try:
                    fs = ModelFrames(dev, kind, 1, 0, None, args.exchange, name=name)
                    es, _ = run_frames(fs, args.steps, args.warmup, dev, None)
                    rec[kind] = {"value": round(args.steps / es, 3), "unit": "frames/s",
                                 "ms_per_step": round(es / args.steps * 1e3, 4), "hip_graph": fs.graph, "build": fs.note,
                                 "protocol_sync": run_frames_protocol(fs, args.steps)}
                    del fs
                    torch.cuda.empty_cache()
                except Exception as exc:
                    rec[kind] = {"error": repr(exc)[:300]}

    frame_roof = {}
    if args.full and not sharded and not args.no_hot_path:
        frame_roof = frame_rooflines(bev, dev)
        torch.cuda.empty_cache()

    bevdet = None
    if args.full and not sharded and not args.no_end_to_end and not args.no_small:
        try:
            bevdet = bevdet_frames(dev, args.steps, args.warmup, not args.no_int8)
        except Exception as exc:
            bevdet = {"error": repr(exc)[:300]}

    if rank == 0:
        cpu = None
        if args.full and not sharded and not args.no_cpu_baseline:
            v, sample = cpu_baseline()
            cpu = {"value": round(v, 5), "unit": "frames/s", "cores": torch.get_num_threads(),
                   "kind": "port",
                   "sample": "the sampling operators of one frame in fp32 on the host (the backbone's dense convolutions, "
                             "GEMMs and norms are NOT in this figure; cpu_baseline.full_model is the whole BEVFormer-tiny): "
                             "MSDA = reference PyTorch CPU path (oracle/torch_ref.py), base TSA, decoder and SCA calls each "
                             "timed whole once, x 6+6+6 calls; DCNv2 = C restatement of the reference launcher "
                             "(oracle/mdconv_ref.c, OpenMP) on one camera image per stage, x 6 images x 23+3 convolutions; "
                             "rotate = oracle/sampler_ref.c once; per-call seconds " + sample}
            try:
                cpu["full_model"] = cpu_full_model()
            except Exception as exc:
                cpu["full_model"] = {"error": repr(exc)[:200]}
        int8 = args.dtype == "int8"
        if headline is not None:
            elapsed = headline["elapsed"]
            metric = (f"frames/sec BEVFormer-base bs=1 {'INT8 (PTQ)' if int8 else 'fp16'} end-to-end on MI355X "
                      "(re-hosted model, random weights, synthetic 6-camera frames)")
            workload = ("BEVFormer-base frame: 6x(3x928x1600) images -> ResNet-101-DCN + FPN -> 6 encoder layers "
                        "(TSA, SCA, FFN; 200x200 BEV queries) -> 6 decoder layers -> heads; prev_bev kept on the device")
            value, ms = args.steps / elapsed, elapsed / args.steps * 1e3
        else:
            metric = f"frames/sec BEVFormer-base bs=1 {'int8' if int8 else 'fp16'} sampling hot path (synthetic)"
            workload = "BEVFormer-base hot path per frame: 26x DCNv2+rotate+6x(TSA+SCA) MSDA+6x decoder MSDA"
            value, ms = hot["value"], hot["ms_per_step"]
        line = {
            "metric": metric, "value": round(value, 3), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms, 4),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "i8" if int8 else "f16", "data": "synthetic",
            "config": {"workload": workload,
                       "shapes": "SCA(6,30825,40000,4x8) TSA(2,40000,40000,1x4) dec(1,40000,900,1x4)",
                       "inputs": "camera images: one synthetic set resident in the frame's static input buffer, replayed "
                                 "every frame (the metric excludes H2D, det2trt/utils/tensorrt.py:69-80); can_bus and "
                                 "lidar2img: fresh values every frame (one 464-byte upload), the camera projection and the "
                                 "SCA visibility plan evaluated from them inside the frame's graph" if headline else None,
                       "dense_dispatch": ("backbone: shipped table (library GEMMs where they measured faster, workspace-free "
                                          "algorithms only); behind the backbone: hand-written kernels only; frames are "
                                          "bit-reproducible run to run") if headline and not sharded else
                                         ("hand-written kernels only (every rank the same choice)" if headline else None),
                       "hip_graph": headline["hip_graph"] if headline else None,
                       "int8_build": headline["note"] if headline else None,
                       # (the stand-alone hot path has no query-sharded encoder: "scatter" runs its all-reduce form there)
                       "parallelism": (f"cameras/{world}+" + (args.exchange if headline is not None or args.exchange == "gather"
                                                              else "reduce")) if sharded else "single"},
            "ranks_seen": dist.get_world_size() if dist is not None else 1,
            "roofline": roofline, "roofline_frame": frame_roof.get("roofline_frame"),
            "roofline_frame_tsa": frame_roof.get("roofline_frame_tsa"), "frame_calibration": frame_roof.get("frame_calibration"),
            "roofline_mfma": frame_roof.get("roofline_mfma"), "cpu_baseline": cpu,
            "hot_path": hot if headline is not None else None,
            "protocol_sync": headline["protocol_sync"] if headline else None,
            "int8": other, "small": small, "tiny": tiny, "bevdet_r50": bevdet,
            "dispatch_misses": dispatch_misses(),
        }
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
