#!/usr/bin/env python3
"""Two (or more) builds of the library against each other on the layers of the 128-row tile family, in ONE process.

Every `--lib name=path` is loaded as a ctypes handle of its own (different files: different copies of the library and
of its kernels).  Per layer shape one HIP graph per build, replayed alternately -- A, B, C, A, B, C, ...: per alternation
the mean of `--replays` replays between two events, then the median, minimum and maximum per arm over `--alternations`
(>= 7) alternations, as tools/yolox_time.py does (means kept to 0.01 us).  Loading the same build twice from two paths gives the noise floor the
comparison is read against.

Shapes are the workload's: every distinct convolution of one YOLOX-x forward at (1, 3, 640, 640) (the list
tools/yolox_time.py --step layers builds), CenterNet-R18's three transposed convolutions at 512 x 512, BEVDepth's ASPP
3 x 3 at dilation 6 on the 6 x 16 x 44 map with 256 channels -- each on the fp16 entry and on its int8 sibling (int8
output where Cout % 16 == 0, else fp16 output; per-channel weight scales).  Operands and launches: tools/tile_family_hash.py.

The measurement is one child process under `timeout`; it stops at the first failure.  One JSON line per shape and entry,
appended to --out.

    python tools/tile_family_ab.py --lib parent=A/libbevops_hip.so --lib parent2=B/libbevops_hip.so \\
        --lib branch=bevformer_tensorrt_amd/libbevops_hip.so [--alternations 7] [--replays 20] [--out ab.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))



def layers():
    """[(label, Case kwargs, fp16 (entry, run kwargs), int8 (entry, run kwargs))]"""
    import torch
    import tile_family_hash as tf
    import yolox_time
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_X
    out = []
    with torch.no_grad():
        model = YOLOX(YOLOX_X, seed=0).cuda().half()
        seen = yolox_time._layer_list(model, (1, 3, 640, 640))
    del model
    torch.cuda.empty_cache()
    for (cin, cout, k, stride, h, w, act, idt) in seen:
        act = act or "none"
        d = tf.I8 if cout % 16 == 0 else tf.F16
        out.append((f"yolox conv {cin} -> {cout} {k}x{k} / {stride} {act}{' + identity' if idt else ''} @ {h}x{w}",
                    dict(kind="conv", B=1, H=h, W=w, cin=cin, cout=cout, k=k, stride=stride, pitched=False),
                    ("bevops_conv_slice_f16", dict(act=act, res=idt)),
                    ("bevops_conv_slice_s8", dict(act=act, res=idt, out_dtype=d))))
    for cin, cout, hw in ((512, 256, 16), (256, 128, 32), (128, 64, 64)):
        out.append((f"centernet deconv {cin} -> {cout} @ {hw}x{hw}",
                    dict(kind="deconv", B=1, H=hw, W=hw, cin=cin, cout=cout, pitched=False),
                    ("bevops_deconv4x4s2_f16", dict(act="relu")), ("bevops_deconv4x4s2_s8", dict(act="relu", out_dtype=tf.I8))))
    out.append(("bevdepth aspp 256 -> 256 3x3 dilation 6 @ 6x16x44",
                dict(kind="conv", B=6, H=16, W=44, cin=256, cout=256, k=3, dilation=6, pitched=False),
                ("bevops_conv_slice_f16_ex", dict(act="relu")), ("bevops_conv_slice_s8_ex2", dict(act="relu", out_dtype=tf.I8))))
    return out


def _alternate(graphs, alternations, replays):
    """{arm: [ms per replay, one value per alternation]}: yolox_time._alternate's scheme, the means kept to 0.01 us (a
    1 % bar on a 13 us layer is 0.13 us)."""
    import yolox_time
    for g in graphs.values():
        yolox_time._replay_ms(g, 3)
    ms = {arm: [] for arm in graphs}
    for _ in range(alternations):
        for arm, g in graphs.items():
            ms[arm].append(round(yolox_time._replay_ms(g, replays), 5))
    return ms


def measure(a):
    import torch
    import tile_family_hash as tf
    import yolox_time
    libs = {}
    for spec in a.lib:
        name, path = spec.split("=", 1)
        libs[name] = tf.load(path)
    dev = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f, torch.no_grad():
        for n, (label, kw, f16, s8) in enumerate(layers()):
            if a.only and a.only not in label:
                continue
            c = tf.Case(seed=n, **kw)
            for entry, rk in (f16, s8):
                outs = {name: tf.run(lib, c, entry, **rk) for name, lib in libs.items()}
                torch.cuda.synchronize()
                first = next(iter(outs.values()))
                equal = all(torch.equal(first.view(torch.uint8), o.view(torch.uint8)) for o in outs.values())
                graphs = {name: yolox_time._capture(lambda lib=lib, o=outs[name]: tf.run(lib, c, entry, out=o, **rk))[0]
                          for name, lib in libs.items()}
                ms = _alternate(graphs, max(7, a.alternations), a.replays)
                rec = {"layer": label, "entry": entry, "args": rk, "rows": c.B * (c.ho * c.wo if c.kind == "conv" else c.H * c.W),
                       "k": c.kk, "cout": c.cout, "outputs_equal": equal, "replays": a.replays, "device": dev}
                for arm, v in ms.items():
                    rec[f"ms_{arm}"] = v
                    rec[f"median_ms_{arm}"] = round(statistics.median(v), 5)
                    rec[f"min_ms_{arm}"] = min(v)
                    rec[f"max_ms_{arm}"] = max(v)
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
                del graphs, outs
            del c
            torch.cuda.empty_cache()
    torch.cuda.synchronize()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", required=True, metavar="NAME=PATH", help="an arm: a build of the library")
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_family", "ab.jsonl"))
    ap.add_argument("--seconds", type=int, default=0,
                    help="time limit of the measuring child; default 600 + 4 per alternation and arm")
    ap.add_argument("--only", default="", help="measure the layers whose label contains this text")
    ap.add_argument("--child", action="store_true", help="measure in this process (what the parent starts under timeout)")
    a = ap.parse_args()
    if a.child:
        return measure(a)
    # (model construction and operands dominate; a record costs alternations x arms x replays launches of 15 - 75 us)
    seconds = a.seconds or 600 + 4 * max(7, a.alternations) * len(a.lib)
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--child", "--alternations",
           str(a.alternations), "--replays", str(a.replays), "--out", a.out, "--only", a.only]
    for spec in a.lib:
        cmd += ["--lib", spec]
    rc = subprocess.run(cmd, cwd=ROOT).returncode
    if rc != 0:
        print(f"the measurement ended with status {rc}", file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
