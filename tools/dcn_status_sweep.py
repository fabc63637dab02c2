#!/usr/bin/env python3
"""The pre-launch status contract of the DCNv2 entries (csrc/mdconv.hip, mdconv_s8.hip), as text: calls each entry of
LIB.so under every accepted bevops_mdconv_set_variant value over a fixed grid of argument tuples -- every pointer NULL /
+2 / +8, every geometry int -1 / 0, channel counts outside each kernel's domain, offset-mask channel counts, dtype codes,
scales 0 / negative / NaN, a short or misaligned workspace, and tuples with two violations at once (which check answers
first) -- and prints one line per call: `entry  v=variant  what differs from the valid base tuple  -> status`.

The pointers are HOST addresses that nothing reads: a tuple that passes every check reaches a device query or a launch,
which without a device fails (status 1).  So the process hides every device from itself before anything loads (below):
no kernel can launch from it, wherever it runs.  Two builds agree on the contract when their outputs are equal line for
line.  --digest prints, per entry, the number of calls per
status and a SHA-256 of the entry's lines (all variants).  --record prints the tuples rejected alike under every
variant (status 2 / 3, and 0 from a size query) as JSON {entry: {label: status}}.

usage: dcn_status_sweep.py LIB.so [--digest | --record | --check RECORDED.json]"""
import collections
import ctypes
import hashlib
import itertools
import json
import math
import os
import sys

os.environ["HIP_VISIBLE_DEVICES"] = os.environ["CUDA_VISIBLE_DEVICES"] = "-1"

F32, F16, I8 = 0, 1, 2            # bevops_dtype_t
VARIANTS = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 14, 15, 20, 24, 25]
P, I, F, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
CTYPES = dict(p=P, stream=P, i=I, f=F, ws_bytes=SZ)

GEO = ["B", "Cin", "H", "W", "Cout", "Kh", "Kw", "sh", "sw", "ph", "pw", "dh", "dw", "G", "DG"]
BASE_GEO = dict(B=1, Cin=128, H=8, W=8, Cout=64, Kh=3, Kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, G=1, DG=1)
# geometries by name: what leaves a kernel's domain, or violates a divisibility rule
SHAPES = {
    "Cin%G": dict(G=3), "Cout%G": dict(G=2, Cout=65), "Cin%DG": dict(DG=3), "Cin%4": dict(Cin=6), "cout_g%4": dict(Cout=6),
    "cin_g%128": dict(Cin=64), "cin_g%64": dict(Cin=96), "3KK>32": dict(Kh=5, Kw=5, ph=2, pw=2), "two_dg": dict(DG=2),
    "groups": dict(G=2, Cin=256, Cout=128), "ragged": dict(Cin=4, Cout=8), "Ho<=0": dict(H=1, W=1, ph=0, pw=0),
    "stride2": dict(sh=2, sw=2), "huge": dict(B=2 ** 20, H=2 ** 10, W=2 ** 10),
}
_G = [(a, "i") for a in GEO] + [("stream", "stream")]
_S8 = [("input", "p"), ("s_in", "f"), ("offset", "p"), ("s_off", "f"), ("mask", "p"), ("s_mask", "f"), ("weight", "p"),
       ("s_w", "f"), ("bias", "p"), ("output", "p"), ("s_out", "f"), ("ws", "p"), ("ws_bytes", "ws_bytes")] + _G
_FP = [("dtype", "i"), ("input", "p"), ("offset", "p"), ("mask", "p"), ("weight", "p"), ("bias", "p"), ("output", "p"),
       ("ws", "p"), ("ws_bytes", "ws_bytes")] + _G
ENTRIES = {
    "bevops_mdconv_forward": dict(args=_FP, dtype=F16),
    "bevops_mdconv_forward_packed": dict(args=_FP, dtype=F16),
    "bevops_mdconv_forward_nhwc": dict(
        args=_FP[:7] + [("relu", "i"), ("om", "i")] + _FP[7:], dtype=F16, om=[0, 26, 27, 28, 31, 32]),
    "bevops_mdconv_forward_int8": dict(args=_S8, dtype=I8),
    "bevops_mdconv_forward_int8_packed": dict(args=_S8, dtype=I8),
    "bevops_mdconv_forward_int8_nhwc": dict(
        args=[("input", "p"), ("s_in", "f"), ("offset", "p"), ("om", "i"), ("s_off", "f"), ("s_mask", "f"), ("weight", "p"),
              ("s_w", "f"), ("bias", "p"), ("output", "p"), ("s_out", "f"), ("relu", "i"), ("exact", "i"), ("ws", "p"),
              ("ws_bytes", "ws_bytes")] + _G, dtype=I8, om=[26, 27, 28, 31, 32], base=dict(om=32)),
    "bevops_mdconv_workspace_size": dict(args=[("dtype", "i")] + _G[:-1], dtype=F16, restype=SZ),
}
# one bad pick per kind of check, combined in pairs (which check answers first)
PAIR_PICKS = [("input", "NULL"), ("output", "+2"), ("weight", "+8"), ("ws", "+2"), ("mask", "NULL"), ("B", 0), ("Kh", -1),
              ("shape", "cin_g%128"), ("shape", "Cin%DG"), ("shape", "3KK>32"), ("shape", "two_dg"), ("shape", "Cin%4"),
              ("shape", "cin_g%64"), ("om", 26), ("om", 27), ("dtype", I8), ("dtype", F32), ("dtype", 3), ("s_in", 0.0),
              ("s_out", math.nan), ("ws_bytes", "size-1"), ("relu", 1)]

_ARENA = ctypes.create_string_buffer(1 << 14)
_ARENA0 = (ctypes.addressof(_ARENA) + 255) & ~255


def spec(name):
    """the entry's base tuple and its axes {argument: values}"""
    e = ENTRIES[name]
    kinds = dict(e["args"])
    base = dict(BASE_GEO, shape="base", **{a: {"p": "A", "f": 1.0, "i": 0, "ws_bytes": "size", "stream": None}[k]
                                           for a, k in e["args"] if a not in BASE_GEO})
    base.update(dtype=e["dtype"], **e.get("base", {}))
    axes = {a: ["NULL", "+2", "+8"] for a, k in e["args"] if k == "p"}
    axes.update({a: [-1, 0] for a in GEO}, shape=list(SHAPES))
    axes.update({a: [0.0, -1.0, math.nan] for a, k in e["args"] if k == "f"})
    if "ws_bytes" in kinds:
        axes["ws_bytes"] = ["size-1", "zero"]
    if "dtype" in kinds:
        axes["dtype"] = [-1, F32, F16, I8, 3]
    for a in ("relu", "exact"):
        if a in kinds:
            axes[a] = [1]
    if "om" in e:
        axes["om"] = e["om"]
    return e, base, axes


def tuples(name):
    """{label: tuple}: the base, every axis value alone, every pair of PAIR_PICKS of two different arguments"""
    e, base, axes = spec(name)
    out = {}

    def add(**change):
        t = dict(base, **change)
        t.update(SHAPES.get(t["shape"], {}))
        label = " ".join(f"{a}={t[a]}" for a in t if a in change and t[a] != base[a])
        out.setdefault(label or "base", t)

    add()
    for a, values in axes.items():
        for v in values:
            add(**{a: v})
    picks = [(a, v) for a, v in PAIR_PICKS if a in axes]
    for (a, va), (b, vb) in itertools.combinations(picks, 2):
        if a != b:
            add(**{a: va, b: vb})
    if "om" in e:       # several deform groups with enough channels for them
        add(shape="two_dg", om=64)
    return out


def call(lib, name, fn, t):
    e, args, slot = ENTRIES[name], [], 0
    for a, k in e["args"]:
        v = t[a]
        if k == "p":
            args.append(None if v == "NULL" else _ARENA0 + 512 * slot + {"A": 0, "+2": 2, "+8": 8}[v])
            slot += 1
        elif k == "ws_bytes":
            size = (lib.bevops_mdconv_int8_nhwc_workspace_size() if name.endswith("int8_nhwc") else
                    lib.bevops_mdconv_workspace_size(t["dtype"], *(t[g] for g in GEO)))
            args.append({"size": size, "size-1": max(size - 1, 0), "zero": 0}[v])
        else:
            args.append(v)
    return fn(*args)


def statuses(lib_path, name, labels=None):
    """(variant, label, status) of the entry's grid, or of the listed labels of it, under every accepted variant"""
    lib = ctypes.CDLL(lib_path)
    lib.bevops_mdconv_workspace_size.restype = lib.bevops_mdconv_int8_nhwc_workspace_size.restype = SZ
    lib.bevops_mdconv_workspace_size.argtypes = [I] * 16
    fn = getattr(lib, name)
    fn.restype = ENTRIES[name].get("restype", I)
    fn.argtypes = [CTYPES[k] for _, k in ENTRIES[name]["args"]]
    grid = tuples(name)
    for v in VARIANTS:
        lib.bevops_mdconv_set_variant(v)
        for label in (grid if labels is None else labels):
            yield v, label, call(lib, name, fn, grid[label])
    lib.bevops_mdconv_set_variant(0)


def main():
    lib_path, mode = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "")
    if mode == "--check":     # against recorded statuses (tests/golden/mdconv_status.json)
        bad = total = 0
        for entry, want in json.load(open(sys.argv[3])).items():
            for v, label, got in statuses(lib_path, "bevops_mdconv_" + entry, list(want)):
                total += 1
                if got != want[label]:
                    bad += 1
                    print(f"{entry}  v={v}  {label}  -> {got}, recorded {want[label]}")
        print(f"# {total} recorded calls, {bad} differ")
        return 1 if bad else 0
    total, record = 0, {}
    for name in ENTRIES:
        entry = name[len("bevops_mdconv_"):]
        got = list(statuses(lib_path, name))
        lines = [f"{entry}  v={v}  {label}  -> {status}" for v, label, status in got]
        total += len(lines)
        if mode == "--digest":
            counts = collections.Counter(status for _, _, status in got)
            print(entry, " ".join(f"status{k}:{n}" for k, n in sorted(counts.items()) if k < 4),
                  "sha256:" + hashlib.sha256("\n".join(lines).encode()).hexdigest())
        elif mode == "--record":
            per = collections.defaultdict(set)
            for _, label, status in got:
                per[label].add(status)
            ok = (0, 2, 3) if "restype" in ENTRIES[name] else (2, 3)
            record[entry] = {label: min(s) for label, s in per.items() if len(s) == 1 and min(s) in ok}
        else:
            print("\n".join(lines))
    if mode == "--record":
        print("{" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in sorted(record.items())) + "}")
    else:
        print(f"# {total} calls, {len(ENTRIES)} entries, {len(VARIANTS)} variants")
    return 0


if __name__ == "__main__":
    sys.exit(main())
