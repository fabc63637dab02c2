#!/usr/bin/env python3
"""The pre-launch status contract of the detection post-processing entries (csrc/decode.hip, decode2d.hip, nms.hip), as
text: calls bevops_nms_free_decode, bevops_centerpoint_decode, bevops_centernet_decode, bevops_yolox_decode,
bevops_bev_nms, bevops_box_nms and the four workspace size queries of LIB.so over a fixed grid of argument tuples --
pointers NULL / misaligned, sizes at and past each limit, bad dtypes, thresholds, factors and strides, and tuples with
two violations at once (which check answers first) -- and prints one line per tuple:
`entry  what differs from the entry's valid base tuple  -> status` (for a size query: the value).

The device pointers are HOST addresses that nothing reads; the host tables (ranges, strides, factors, borders, level
tables) are real.  A tuple that passes every check reaches the launch, which without a device fails (status 1).  So
this tool runs only where no kernel can launch, and refuses to start where torch sees a device.  Two builds agree on the
contract when their outputs are equal line for line.  Each entry's sweep runs in a child process.

usage: postprocess_status_sweep.py LIB.so [--digest | --entry NAME | --record OUT.json | --check RECORDED.json]
--record keeps the rejected tuples (status 2 or 3) and every size-query value; --digest prints, per entry, the number
of tuples per answer and a SHA-256 of the entry's lines instead of the lines."""
import collections
import ctypes
import hashlib
import itertools
import json
import math
import subprocess
import sys

F32, F16, I8 = 0, 1, 2            # bevops_dtype_t
P, I, F, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
NAN, INF = math.nan, math.inf

_ARENA = ctypes.create_string_buffer(1 << 16)
_ARENA0 = (ctypes.addressof(_ARENA) + 255) & ~255


def ptr(slot, how):
    """host address of pointer argument number `slot`: 256-byte aligned, moved by +4 bytes, or NULL"""
    return None if how == "NULL" else _ARENA0 + 512 * slot + {"A": 0, "+4": 4}[how]


def floats(values):
    return (ctypes.c_float * len(values))(*values)


def ints(values):
    return (ctypes.c_int32 * len(values))(*values)


# host tables by name
TABLES = {
    "range": lambda: floats([-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]),
    "ones12": lambda: ints([1] * 12), "zero_at_0": lambda: ints([0] + [1] * 11), "neg_at_11": lambda: ints([1] * 11 + [-1]),
    "zero_at_5": lambda: ints([1] * 5 + [0] + [1] * 6),
    "fac": lambda: floats([1.0] * 64), "fac_zero": lambda: floats([1.0, 0.0] + [1.0] * 62),
    "fac_nan": lambda: floats([NAN] + [1.0] * 63), "fac_neg": lambda: floats([1.0] * 63 + [-2.0]),
    "border": lambda: floats([0.0] * 128), "border_inf": lambda: floats([0.0, INF] + [0.0] * 126),
    "scale": lambda: floats([1.0] * 256), "scale_zero": lambda: floats([1.0] * 5 + [0.0] + [1.0] * 250),
    "scale_nan": lambda: floats([NAN] + [1.0] * 255),
    "levels": lambda: ints([80, 80, 8, 40, 40, 16, 20, 20, 32] + [1, 1, 1] * 5),
    "levels_h0": lambda: ints([80, 80, 8, 0, 40, 16, 20, 20, 32] + [1, 1, 1] * 5),
    "levels_stride0": lambda: ints([80, 80, 0, 40, 40, 16, 20, 20, 32] + [1, 1, 1] * 5),
    "levels_big": lambda: ints([4096, 4096, 8, 4096, 1, 16, 20, 20, 32] + [1, 1, 1] * 5),
    "levels_sum_big": lambda: ints([4096, 2048, 8, 4096, 2048, 16, 20, 20, 32] + [1, 1, 1] * 5),
    "ones48": lambda: ints([1] * 48), "zero_at_7": lambda: ints([1] * 7 + [0] + [1] * 40),
    "ptrs": lambda: (P * 8)(*[ptr(20 + i, "A") for i in range(8)]),
    "ptrs_null1": lambda: (P * 8)(*[ptr(20 + i, "A" if i != 1 else "NULL") for i in range(8)]),
}

PTRS = ["A", "NULL"]
WS = ["A", "NULL", "+4"]
WSB = ["size", "size-1", "zero"]
DTYPES = [F32, F16, I8, 7, -1]

# (argument, kind) in C order.  kinds: p pointer into the arena, i / f scalars, t named host table (or NULL), ws the
# workspace pointer, wsb its size relative to the size query, stream (always NULL)
OUT4 = [("boxes", "p"), ("scores", "p"), ("labels", "p"), ("count", "p")]
NMS_IO = [("boxes_in", "p"), ("scores_in", "p"), ("labels_in", "p"), ("count_in", "p")] + OUT4 + [("index", "p")]
ENTRIES = {
    "bevops_nms_free_decode": dict(
        args=[("dtype", "i"), ("cls", "p"), ("bbox", "p")] + OUT4 + [("batch", "i"), ("nq", "i"), ("nc", "i"), ("max_num", "i"),
              ("range", "t"), ("thr", "f"), ("bottom", "i"), ("stream", "stream")],
        base=dict(dtype=F32, batch=1, nq=900, nc=10, max_num=300, range="range", thr=-1.0, bottom=0),
        axes=dict(dtype=DTYPES, batch=[-1, 0, 1, 65535, 65536], nq=[0, 900, 1639, 16384, 16385], nc=[0, 1, 10, 11],
                  max_num=[0, 1, 300, 9000, 9001, 16384, 16385], range=["range", "NULL"], thr=[-1.0, 0.3, NAN, INF, 3.0e38],
                  bottom=[0, 1]),
        bad=dict(dtype=[I8, 7], batch=[0, 65536], nq=[0, 16385], nc=[0], max_num=[0, 9001, 16385], range=["NULL"],
                 thr=[NAN, INF])),
    "bevops_centerpoint_decode_workspace_size": dict(
        args=[("batch", "i"), ("nc", "i"), ("H", "i"), ("W", "i"), ("max_num", "i")], restype=SZ,
        base=dict(batch=1, nc=10, H=128, W=128, max_num=500),
        grid=dict(batch=[-1, 0, 1, 6, 65535, 65536], nc=[0, 1, 10], H=[0, 1, 20, 64, 128], W=[1, 128, 205, 1 << 14],
                  max_num=[0, 1, 500, 4096, 4097])),
    "bevops_centerpoint_decode": dict(
        args=[("dtype", "i"), ("reg", "p"), ("height", "p"), ("dim", "p"), ("rot", "p"), ("vel", "p"), ("heat", "p"),
              ("strides", "t")] + OUT4 + [("batch", "i"), ("nc", "i"), ("H", "i"), ("W", "i"), ("max_num", "i"), ("osf", "f"),
              ("vx", "f"), ("vy", "f"), ("pcx", "f"), ("pcy", "f"), ("range", "t"), ("thr", "f"), ("norm", "i"), ("his", "i"),
              ("ws", "ws"), ("wsb", "wsb"), ("stream", "stream")],
        size=("bevops_centerpoint_decode_workspace_size", ("batch", "nc", "H", "W", "max_num")),
        base=dict(dtype=F16, strides="ones12", batch=1, nc=10, H=128, W=128, max_num=500, osf=8.0, vx=0.1, vy=0.1, pcx=-51.2,
                  pcy=-51.2, range="range", thr=0.1, norm=1, his=0, ws="A", wsb="size"),
        axes=dict(dtype=DTYPES, strides=["ones12", "zero_at_0", "neg_at_11", "NULL"], batch=[-1, 0, 1, 65535, 65536],
                  nc=[0, 1, 10], H=[0, 1, 20, 128, 1 << 15], W=[0, 1, 128, 1 << 15], max_num=[0, 1, 500, 4096, 4097],
                  range=["range", "NULL"], thr=[-1.0, 0.1, NAN, INF], ws=WS, wsb=WSB),
        bad=dict(dtype=[I8, 7], strides=["zero_at_0", "NULL"], batch=[0, 65536], nc=[0], H=[0, 1 << 15], max_num=[0, 4097],
                 range=["NULL"], thr=[NAN], ws=["NULL", "+4"], wsb=["size-1"]),
        null_ok=("reg", "vel")),
    "bevops_centernet_decode_workspace_size": dict(
        args=[("batch", "i"), ("nc", "i"), ("H", "i"), ("W", "i"), ("k", "i")], restype=SZ,
        base=dict(batch=1, nc=80, H=128, W=128, k=100),
        grid=dict(batch=[-1, 0, 1, 64, 65], nc=[0, 1, 80, 1 << 13], H=[0, 1, 128, 2048, 4096], W=[1, 128, 2048],
                  k=[0, 1, 100, 4096, 4097])),
    "bevops_centernet_decode": dict(
        args=[("dtype", "i"), ("heat", "p"), ("wh", "p"), ("off", "p"), ("strides", "t")] + OUT4 +
             [("batch", "i"), ("nc", "i"), ("H", "i"), ("W", "i"), ("k", "i"), ("kernel", "i"), ("inp_h", "i"), ("inp_w", "i"),
              ("border", "t"), ("scale", "t"), ("thr", "f"), ("ws", "ws"), ("wsb", "wsb"), ("stream", "stream")],
        size=("bevops_centernet_decode_workspace_size", ("batch", "nc", "H", "W", "k")),
        base=dict(dtype=F32, strides="ones12", batch=2, nc=80, H=128, W=128, k=100, kernel=3, inp_h=512, inp_w=512,
                  border="border", scale="scale", thr=-1.0, ws="A", wsb="size"),
        axes=dict(dtype=DTYPES, strides=["ones12", "zero_at_0", "zero_at_5", "NULL"], batch=[-1, 0, 1, 64, 65],
                  nc=[0, 1, 80, 1 << 13], H=[0, 1, 128, 4096], W=[0, 128, 2048], k=[-1, 0, 1, 100, 4096, 4097],
                  kernel=[0, 1, 2, 3, 7, 9], inp_h=[0, 512], inp_w=[0, 512], border=["border", "border_inf", "NULL"],
                  scale=["scale", "scale_zero", "scale_nan", "NULL"], thr=[-1.0, 0.3, NAN, INF], ws=WS, wsb=WSB),
        bad=dict(dtype=[I8, 7], strides=["zero_at_5", "NULL"], batch=[0, 65], nc=[0, 1 << 13], H=[0, 4096], k=[0, 4097],
                 kernel=[0, 2, 9], inp_w=[0], border=["border_inf"], scale=["scale_zero", "scale_nan"], thr=[NAN],
                 ws=["NULL", "+4"], wsb=["size-1"])),
    "bevops_yolox_decode": dict(
        args=[("dtype", "i"), ("cls", "t"), ("bbox", "t"), ("obj", "t"), ("levels", "t"), ("strides", "t"), ("boxes", "p"),
              ("scores", "p"), ("labels", "p"), ("batch", "i"), ("nl", "i"), ("nc", "i"), ("scale", "t"), ("stream", "stream")],
        base=dict(dtype=F16, cls="ptrs", bbox="ptrs", obj="ptrs", levels="levels", strides="ones48", batch=1, nl=3, nc=80,
                  scale="scale"),
        axes=dict(dtype=DTYPES, cls=["ptrs", "ptrs_null1", "NULL"], bbox=["ptrs", "ptrs_null1", "NULL"],
                  obj=["ptrs", "ptrs_null1", "NULL"], levels=["levels", "levels_h0", "levels_stride0", "levels_big",
                                                             "levels_sum_big", "NULL"],
                  strides=["ones48", "zero_at_7", "NULL"], batch=[-1, 0, 1, 64, 65], nl=[-1, 0, 1, 3, 8, 9], nc=[0, 1, 80],
                  scale=["scale", "scale_zero", "scale_nan", "NULL"]),
        bad=dict(dtype=[I8, 7], cls=["ptrs_null1", "NULL"], obj=["ptrs_null1"], levels=["levels_h0", "levels_big",
                                                                                      "levels_sum_big", "NULL"],
                 strides=["zero_at_7", "NULL"], batch=[0, 65], nl=[0, 9], nc=[0], scale=["scale_zero", "scale_nan"])),
    "bevops_bev_nms_workspace_size": dict(
        args=[("batch", "i"), ("num", "i")], restype=SZ, base=dict(batch=1, num=500),
        grid=dict(batch=[-1, 0, 1, 2, 3, 6, 65535, 65536], num=[-1, 0, 1, 2, 3, 63, 64, 65, 83, 500, 1000, 4095, 4096, 4097])),
    "bevops_bev_nms": dict(
        args=[("mode", "i")] + NMS_IO + [("batch", "i"), ("num", "i"), ("pre", "i"), ("post", "i"), ("thr", "f"), ("fac", "t"),
              ("nfac", "i"), ("bottom", "i"), ("ws", "ws"), ("wsb", "wsb"), ("stream", "stream")],
        size=("bevops_bev_nms_workspace_size", ("batch", "num")),
        base=dict(mode=0, batch=1, num=500, pre=0, post=83, thr=0.2, fac="fac", nfac=10, bottom=0, ws="A", wsb="size"),
        axes=dict(mode=[-1, 0, 1, 2], batch=[-1, 0, 1, 65535, 65536], num=[-1, 0, 1, 82, 83, 500, 4096, 4097],
                  pre=[-5, 0, 1, 100, 500, 9999], post=[-1, 0, 1, 83, 500, 501], thr=[0.0, 0.2, -1.0, NAN, INF, -INF],
                  fac=["fac", "fac_zero", "fac_nan", "fac_neg", "NULL"], nfac=[-1, 0, 1, 2, 10, 64, 65], bottom=[0, 1], ws=WS,
                  wsb=WSB),
        bad=dict(mode=[2], batch=[0, 65536], num=[0, 82, 4097], post=[0, 501], thr=[NAN, INF], fac=["fac_zero", "fac_nan", "NULL"],
                 nfac=[-1, 64, 65], ws=["NULL", "+4"], wsb=["size-1"]),
        null_ok=("count_in", "index")),
    "bevops_box_nms_workspace_size": dict(
        args=[("batch", "i"), ("num", "i")], restype=SZ, base=dict(batch=1, num=8400),
        grid=dict(batch=[-1, 0, 1, 2, 3, 6, 65535, 65536], num=[-1, 0, 1, 2, 3, 63, 64, 65, 100, 1000, 8400, 16383, 16384, 16385])),
    "bevops_box_nms": dict(
        args=NMS_IO + [("batch", "i"), ("num", "i"), ("sthr", "f"), ("thr", "f"), ("aware", "i"), ("max_out", "i"), ("ws", "ws"),
                       ("wsb", "wsb"), ("stream", "stream")],
        size=("bevops_box_nms_workspace_size", ("batch", "num")),
        base=dict(batch=1, num=8400, sthr=0.01, thr=0.65, aware=1, max_out=100, ws="A", wsb="size"),
        axes=dict(batch=[-1, 0, 1, 65535, 65536], num=[-1, 0, 1, 99, 100, 8400, 16384, 16385], sthr=[-INF, 0.01, NAN, INF],
                  thr=[0.0, 0.65, -1.0, NAN, INF], aware=[-1, 0, 1, 2], max_out=[-1, 0, 1, 100, 8400, 8401], ws=WS, wsb=WSB),
        bad=dict(batch=[0, 65536], num=[0, 99, 16385], sthr=[NAN], thr=[NAN, INF], aware=[2], max_out=[0, 8401],
                 ws=["NULL", "+4"], wsb=["size-1"]),
        null_ok=("count_in", "index")),
}
CTYPES = dict(p=P, t=P, ws=P, stream=P, i=I, f=F, wsb=SZ)


def show(v):
    return "nan" if isinstance(v, float) and v != v else str(v)


def tuples(e):
    """the entry's grid as {label: tuple}: the base, every axis value alone (every pointer also NULL), every pair of bad
    picks of two different arguments; for a size query the full product of its grid"""
    base = {a: ("A" if k in ("p", "ws") else None) for a, k in e["args"]}
    base.update(e["base"])
    out = {}

    def add(**change):
        t = dict(base, **change)
        label = " ".join(f"{a}={show(t[a])}" for a, _ in e["args"] if show(t[a]) != show(base[a]))
        out.setdefault(label or "base", t)

    add()
    if "grid" in e:
        names = list(e["grid"])
        for combo in itertools.product(*(e["grid"][a] for a in names)):
            add(**dict(zip(names, combo)))
        return out
    axes, bad = dict(e["axes"]), dict(e["bad"])
    for a, k in e["args"]:
        if k == "p":
            axes[a] = PTRS
            if a not in e.get("null_ok", ()):
                bad[a] = ["NULL"]
    for a, values in axes.items():
        for v in values:
            add(**{a: v})
    picks = [(a, v) for a, values in bad.items() for v in values]
    for (a, va), (b, vb) in itertools.combinations(picks, 2):
        if a != b:
            add(**{a: va, b: vb})
    return out


def bind(lib, name):
    fn = getattr(lib, name)
    fn.restype = ENTRIES[name].get("restype", I)
    fn.argtypes = [CTYPES[k] for _, k in ENTRIES[name]["args"]]
    return fn


def call(fn, size_fn, e, t):
    args, keep = [], []
    for slot, (a, k) in enumerate(e["args"]):
        v = t[a]
        if k in ("p", "ws"):
            args.append(ptr(slot, v))
        elif k == "stream":
            args.append(None)
        elif k == "t":
            tab = None if v == "NULL" else TABLES[v]()
            keep.append(tab)
            args.append(ctypes.cast(tab, P) if tab is not None else None)
        elif k == "wsb":
            size = size_fn(*(t[x] for x in e["size"][1]))
            args.append({"size": size, "size-1": max(size - 1, 0), "zero": 0}[v])
        else:
            args.append(v)
    return fn(*args)


def statuses(lib_path, name, labels=None):
    """(label, status or size) of the entry's grid, or of the listed labels of it"""
    lib = ctypes.CDLL(lib_path)
    e = ENTRIES[name]
    fn = bind(lib, name)
    size_fn = bind(lib, e["size"][0]) if "size" in e else None
    grid = tuples(e)
    for label in (grid if labels is None else labels):
        yield label, call(fn, size_fn, e, grid[label])


def sweep(lib_path):
    """{entry: [(label, value)]}, one child process per entry; None for an entry whose child failed"""
    out = {}
    for name in ENTRIES:
        r = subprocess.run([sys.executable, __file__, lib_path, "--entry", name], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            out[name] = None
            continue
        out[name] = [(ln.split("  ", 1)[1].rsplit("  -> ", 1)[0], int(ln.rsplit(" ", 1)[1])) for ln in r.stdout.splitlines()]
    return out


def check(lib_path, golden_path):
    """compare the library against the recorded values (tests/golden/postprocess_status.json: per entry {label: status}
    of its rejected tuples, per size query the values of its whole grid in the grid's order)"""
    bad = total = 0
    for short, want in json.load(open(golden_path)).items():
        if isinstance(want, list):
            labels = list(tuples(ENTRIES["bevops_" + short]))
            assert len(labels) == len(want), f"{short}: {len(want)} recorded values for a grid of {len(labels)}"
            want = dict(zip(labels, want))
        for label, got in statuses(lib_path, "bevops_" + short, list(want)):
            total += 1
            if got != want[label]:
                bad += 1
                print(f"{short}  {label}  -> {got}, recorded {want[label]}")
    print(f"# {total} recorded tuples, {bad} differ")
    return 1 if bad else 0


def main():
    import torch
    if torch.cuda.is_available():
        print("postprocess_status_sweep.py passes host pointers: it must not run where a kernel could launch")
        return 3
    lib_path, mode = sys.argv[1], (sys.argv[2] if len(sys.argv) > 3 else None)
    if mode == "--check":
        return check(lib_path, sys.argv[3])
    if mode == "--entry":
        for label, status in statuses(lib_path, sys.argv[3]):
            print(f"{sys.argv[3][len('bevops_'):]}  {label}  -> {status}")
        return 0
    table = sweep(lib_path)
    failed = [n for n, rows in table.items() if rows is None]
    if mode == "--record":
        kept = {n[len("bevops_"):]: [v for _, v in rows] if "restype" in ENTRIES[n] else {label: v for label, v in rows if v in (2, 3)}
                for n, rows in table.items() if rows is not None}
        with open(sys.argv[3], "w") as f:        # one line per entry
            f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(t, separators=(',', ':'))}" for n, t in sorted(kept.items())) + "\n}\n")
        print(f"# recorded {sum(len(t) for t in kept.values())} tuples of {len(kept)} entries")
    elif "--digest" in sys.argv[2:]:      # per entry the number of tuples per answer and one hash of its lines
        for n, rows in table.items():
            lines = "".join(f"{n[len('bevops_'):]}  {label}  -> {v}\n" for label, v in rows or ())
            counts = collections.Counter("value" if "restype" in ENTRIES[n] else f"status{v}" for _, v in rows or ())
            print(n[len("bevops_"):], " ".join(f"{k}:{c}" for k, c in sorted(counts.items())),
                  "sha256:" + hashlib.sha256(lines.encode()).hexdigest())
        print(f"# {sum(len(r or ()) for r in table.values())} tuples, {len(ENTRIES)} entries")
    else:
        for n, rows in table.items():
            for label, v in rows or ():
                print(f"{n[len('bevops_'):]}  {label}  -> {v}")
            if rows is None:
                print(f"{n[len('bevops_'):]}  CHILD FAILED")
        print(f"# {sum(len(r or ()) for r in table.values())} tuples, {len(ENTRIES)} entries")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
