#!/usr/bin/env python3
"""The pre-launch status contract of every dense GEMM entry, as text: calls each entry of LIB.so over a fixed grid of
argument tuples -- pointers NULL / aligned / +2 / +8, the row, column and depth counts inside and outside every domain,
scales, dtype codes, group strides, destination tables, and tuples with two violations at once (which check answers
first) -- and prints one line per tuple: `entry  what differs from the entry's valid base tuple  -> status`.

The pointers are HOST addresses that nothing reads (except the shape and destination tables, which are real): a tuple
that passes every check reaches the launch, which without a device fails (status 1).  So this tool runs only where no
kernel can launch, and refuses to start where torch sees a device.  Two builds agree on the contract when their outputs
are equal line for line.  Each entry's sweep runs in a child process: a crash costs that entry's lines only.
--digest prints, per entry, the number of tuples per status and a SHA-256 of the entry's lines instead of the lines.

usage: gemm_status_sweep.py LIB.so [--digest | --entry NAME | --check RECORDED.json]"""
import collections
import ctypes
import hashlib
import itertools
import math
import subprocess
import sys

F32, F16, I8 = 0, 1, 2            # bevops_dtype_t
P, LL, I, F, SZ = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_float, ctypes.c_size_t

M_VALUES = [-1, 0, 1, 64, 65537, 2 ** 31]
N_VALUES = [0, 8, 64, 72, 96, 256, 512]
K_VALUES = [0, 8, 64, 100, 128, 256, 320, 1024, 1088]
PTR_VALUES = ["A", "NULL", "+2", "+8"]


class GemmDst(ctypes.Structure):     # bevops_gemm_dst (include/bevops.h)
    _fields_ = [("col_begin", I), ("col_end", I), ("out", P), ("out_pitch", LL), ("res", P), ("res_pitch", LL)]


_ARENA = ctypes.create_string_buffer(1 << 16)
_ARENA0 = (ctypes.addressof(_ARENA) + 255) & ~255


def ptr(slot, how):
    """host address of pointer argument number `slot`: 256-byte aligned, moved by +2 / +8 bytes, or NULL"""
    if how == "NULL":
        return None
    return _ARENA0 + 512 * slot + {"A": 0, "+2": 2, "+8": 8, "+64": 64}[how]


# destination tables by name: rows of (col_begin, col_end, out, out_pitch, res, res_pitch)
def _t(*rows):
    return [r if len(r) == 6 else r + ("NULL", 0) for r in rows]


DST_TABLES = {
    "ok2": _t((0, 64, "A", 64), (64, 128, "A", 64)),
    "ok2_res": _t((0, 64, "A", 64, "A", 64), (64, 128, "A", 128, "A", 72)),
    "ok1": _t((0, 128, "A", 128)),
    "end8": _t((0, 64, "A", 64), (64, 96, "A", 32)),
    "end8_res": _t((0, 64, "A", 64, "A", 64), (64, 96, "A", 32, "A", 32)),
    "end4": _t((0, 60, "A", 64)),
    "begin8": _t((8, 64, "A", 64)),
    "begin_neg": _t((-64, 64, "A", 128)),
    "end_past_n": _t((0, 1024, "A", 1024)),
    "empty": _t((64, 64, "A", 64)),
    "reversed": _t((64, 0, "A", 64)),
    "overlap": _t((0, 128, "A", 128), (64, 128, "A", 64)),
    "same_range": _t((0, 64, "A", 64), (0, 64, "A", 64)),
    "share_block": _t((0, 72, "A", 72), (64, 96, "A", 32)),
    "share_block_rev": _t((64, 96, "A", 32), (0, 72, "A", 72)),
    "pitch_short": _t((0, 64, "A", 56)),
    "pitch_odd": _t((0, 64, "A", 68)),
    "pitch_65": _t((0, 64, "A", 65)),
    "pitch_2p31": _t((0, 64, "A", 2 ** 31)),
    "res_pitch_short": _t((0, 64, "A", 64, "A", 56)),
    "res_pitch_odd": _t((0, 64, "A", 64, "A", 68)),
    "res_pitch_2p31": _t((0, 64, "A", 64, "A", 2 ** 31)),
    "res_pitch_big": _t((0, 64, "A", 64, "A", 2 ** 31 - 8)),
    "res_pitch_32768": _t((0, 64, "A", 64, "A", 32768)),
    "out_null": _t((0, 64, "NULL", 64)),
    "out+2": _t((0, 64, "+2", 64)),
    "out+8": _t((0, 64, "+8", 64)),
    "res+2": _t((0, 64, "A", 64, "+2", 64)),
    "res+8": _t((0, 64, "A", 64, "+8", 64)),
    "res_null_pitch_bad": _t((0, 64, "A", 64, "NULL", 3)),
    "second_bad_after_big_res": _t((0, 64, "A", 64, "A", 2 ** 31 - 8), (64, 100, "A", 64)),
    "second_out+2": _t((0, 64, "A", 64), (64, 128, "+2", 64)),
    "nine": _t(*[(64 * i, 64 * i + 64, "A", 64) for i in range(9)]),
    "eight": _t(*[(64 * i, 64 * i + 64, "A", 64) for i in range(8)]),
}


def dst_table(name, count):
    """(ctypes array or None, num_dst) of the named table; `count` overrides the number of entries passed"""
    if name == "NULL":
        return None, (1 if count is None else count)
    rows = DST_TABLES[name]
    tab = (GemmDst * len(rows))()
    for i, (b, e, out, op, res, rp) in enumerate(rows):
        tab[i] = GemmDst(b, e, ptr(16 + 2 * i, out), op, ptr(17 + 2 * i, res), rp)
    return tab, (len(rows) if count is None else count)


SHAPES = {"tiny": [[116, 200], [58, 100], [29, 50], [15, 25]], "base": [[58, 100], [29, 50], [15, 25], [8, 13]],
          "one": [[1, 1], [1, 1], [1, 1], [1, 1]]}


def shapes_array(name):
    if name == "NULL":
        return None, 0
    flat = [v for hw in SHAPES[name] for v in hw]
    return (ctypes.c_int32 * len(flat))(*flat), sum(h * w for h, w in SHAPES[name])


# ---- the entries: (argument name, kind) in C order.  kinds: p pointer into the arena, ll / i / f / sz scalars,
# stream (always NULL), dst + ndst (destination table), shapes (int32 host table), gstride (named, relative to m * 256),
# nk / pbytes (named, relative to the shape table / the size query)
def _gemm(*front):
    return list(front) + [("m", "ll"), ("n", "i"), ("k", "i")]


S8_HEAD = [("a", "p"), ("sa", "f"), ("w", "p"), ("wsc", "p"), ("sw", "f"), ("bias", "p"), ("res", "p")]
CONV_DIMS = [("B", "i"), ("H", "i"), ("W", "i"), ("Cin", "i"), ("Cout", "i"), ("ks", "i"), ("stride", "i"), ("relu", "i"),
             ("stream", "stream")]
F16_HEAD = [("x", "p"), ("w", "p"), ("bias", "p"), ("res", "p"), ("out", "p")]
PACK_DIMS = [("cams", "i"), ("nk", "nk"), ("heads", "i"), ("ch", "i"), ("levels", "i"), ("nq", "i"), ("np", "i")]

ENTRIES = {
    "bevops_tsgemm_f16": dict(args=_gemm(*F16_HEAD) + [("relu", "i"), ("stream", "stream")], base=dict(m=64, n=256, k=64)),
    "bevops_tsgemm_f16_grouped": dict(
        args=[("x", "p"), ("w", "p"), ("bias", "p"), ("out", "p"), ("gstride", "gstride"), ("m", "ll"), ("groups", "i"),
              ("k", "i"), ("stream", "stream")],
        base=dict(m=64, groups=2, k=64, gstride="equal"),
        axes=dict(gstride=["equal", "below", "unaligned", "above"], groups=[-1, 0, 1, 2, 64, 65]), dims=dict(m=M_VALUES, k=K_VALUES),
        bad=dict(gstride=["below", "unaligned"], groups=[0, 65])),
    "bevops_tsgemm_f16_ln": dict(
        args=[("x", "p"), ("w", "p"), ("bias", "p"), ("res", "p"), ("lnw", "p"), ("lnb", "p"), ("eps", "f"), ("out", "p"),
              ("m", "ll"), ("n", "i"), ("k", "i"), ("stream", "stream")],
        base=dict(m=64, n=256, k=64, eps=1e-5), axes=dict(eps=[-1.0, 0.0, 1e-5, math.nan]), bad=dict(eps=[-1.0, math.nan])),
    "bevops_tsgemm_s8": dict(
        args=S8_HEAD + [("res_dtype", "i"), ("sres", "f"), ("out_dtype", "i"), ("out", "p"), ("sout", "f"), ("m", "ll"),
                        ("n", "i"), ("k", "i"), ("relu", "i"), ("stream", "stream")],
        base=dict(m=64, n=256, k=128), int8=("sa", "sw", "sres", "sout")),
    "bevops_tsgemm_s8_ln": dict(
        args=S8_HEAD + [("res_dtype", "i"), ("sres", "f"), ("lnw", "p"), ("lnb", "p"), ("eps", "f"), ("out", "p"), ("m", "ll"),
                        ("n", "i"), ("k", "i"), ("stream", "stream")],
        base=dict(m=64, n=256, k=128, eps=1e-5), axes=dict(eps=[-1.0, 0.0, 1e-5, math.nan]), bad=dict(eps=[-1.0, math.nan]),
        int8=("sa", "sw", "sres")),
    "bevops_value_proj_packed_size": dict(
        args=[("shapes", "shapes")] + PACK_DIMS, restype=SZ,
        base=dict(shapes="tiny", cams=6, nk="sum", heads=8, ch=32, levels=4, nq=2500, np=8),
        axes=dict(shapes=["tiny", "base", "one", "NULL"], cams=[-1, 0, 1, 6, 2 ** 20], nk=["sum", "sum-1", "zero"],
                  heads=[0, 4, 8, 16, 24], ch=[16, 32, 64], levels=[1, 3, 4], nq=[0, 2500, 40000], np=[4, 8, 16]),
        dims={}, bad=dict(shapes=["NULL"], cams=[0, 2 ** 20], nk=["sum-1", "zero"], heads=[0, 4], ch=[64], levels=[3], np=[4])),
    "bevops_value_proj_packed": dict(
        args=[("x", "p"), ("w", "p"), ("bias", "p"), ("shapes", "shapes"), ("packed", "p"), ("pbytes", "pbytes")] + PACK_DIMS +
             [("stream", "stream")],
        base=dict(shapes="tiny", cams=6, nk="sum", heads=8, ch=32, levels=4, nq=2500, np=8, pbytes="size"),
        axes=dict(shapes=["tiny", "base", "one", "NULL"], cams=[-1, 0, 1, 6, 2 ** 20], nk=["sum", "sum-1", "zero"],
                  heads=[0, 4, 8, 16, 24], ch=[16, 32, 64], levels=[1, 3, 4], nq=[0, 2500, 40000], np=[4, 8, 16],
                  pbytes=["size", "size-1", "zero"], packed=["A", "NULL", "+2", "+8", "+64"]),
        dims={}, bad=dict(shapes=["NULL"], cams=[0, 2 ** 20], nk=["sum-1", "zero"], heads=[0, 4], ch=[64], levels=[3], np=[4],
                          pbytes=["size-1"], packed=["NULL", "+64"])),
    "bevops_tile_gemm_f16": dict(args=_gemm(*F16_HEAD) + [("relu", "i"), ("stream", "stream")], base=dict(m=64, n=256, k=64)),
    "bevops_tile_gemm_f16_dst": dict(
        args=[("x", "p"), ("w", "p"), ("bias", "p"), ("dst", "dst"), ("ndst", "ndst"), ("m", "ll"), ("n", "i"), ("k", "i"),
              ("relu", "i"), ("stream", "stream")],
        base=dict(m=64, n=128, k=64, dst="ok2"), tables=True),
    "bevops_linear_int8": dict(
        args=S8_HEAD + [("out_dtype", "i"), ("out", "p"), ("sout", "f"), ("m", "ll"), ("n", "i"), ("k", "i"), ("relu", "i"),
                        ("stream", "stream")],
        base=dict(m=64, n=256, k=64), int8=("sa", "sw", "sout")),
    "bevops_linear_int8_fused": dict(
        args=S8_HEAD + [("out_dtype", "i"), ("out", "p"), ("sout", "f"), ("m", "ll"), ("n", "i"), ("k", "i"), ("relu", "i"),
                        ("stream", "stream")],
        base=dict(m=64, n=256, k=64), int8=("sa", "sw", "sout")),
    "bevops_linear_int8_chain": dict(
        args=[("a", "p"), ("a_dtype", "i"), ("sa", "f"), ("w", "p"), ("wsc", "p"), ("sw", "f"), ("bias", "p"), ("res", "p"),
              ("res_dtype", "i"), ("sres", "f"), ("out_dtype", "i"), ("out", "p"), ("sout", "f"), ("m", "ll"), ("n", "i"),
              ("k", "i"), ("relu", "i"), ("stream", "stream")],
        base=dict(m=64, n=256, k=64, a_dtype=I8), int8=("sa", "sw", "sres", "sout")),
    "bevops_conv_tile_int8_fused": dict(args=S8_HEAD + [("out", "p")] + CONV_DIMS, conv=64, int8=("sa", "sw")),
    "bevops_conv_tile_f16": dict(args=F16_HEAD + CONV_DIMS, conv=32),
    "bevops_conv_tile_int8": dict(args=S8_HEAD + [("out_dtype", "i"), ("out", "p"), ("sout", "f")] + CONV_DIMS, conv=64,
                                  int8=("sa", "sw", "sout")),
    "bevops_small_gemm_f16": dict(args=_gemm(*F16_HEAD) + [("relu", "i"), ("stream", "stream")], base=dict(m=64, n=256, k=64)),
    "bevops_small_gemm_f16_dst": dict(
        args=[("x", "p"), ("w", "p"), ("bias", "p"), ("dst", "dst"), ("ndst", "ndst"), ("m", "ll"), ("n", "i"), ("k", "i"),
              ("relu", "i"), ("stream", "stream")],
        base=dict(m=64, n=128, k=64, dst="ok2"), tables=True),
}

DEFAULTS = dict(p="A", f=1.0, i=0, ll=0, stream=None, ndst=None, res_dtype=F16, out_dtype=F16)
BAD_DIMS = dict(m=[-1, 0, 65537, 2 ** 31], n=[0, 72, 96], k=[0, 8, 100, 320, 1088])


def spec(name):
    """the entry's description with its base tuple, its axes (every value of every swept argument), its dims (swept as a
    full product) and its bad picks (combined in pairs) filled in"""
    e = dict(ENTRIES[name])
    kinds = dict(e["args"])
    base = {a: DEFAULTS.get(a, DEFAULTS.get(k)) for a, k in e["args"]}
    axes, bad = {}, {}
    if "conv" in e:
        base.update(B=1, H=8, W=8, Cin=64, Cout=64, ks=3, stride=1)
        axes.update(B=[-1, 0, 1, 2 ** 20], H=[0, 1, 8, 2 ** 12], W=[0, 8, 2 ** 12], Cin=[0, 16, 32, 64, 96], Cout=[0, 8, 64, 72, 256],
                    ks=[0, 1, 2, 3, 5], stride=[0, 1, 2, 3])
        bad.update(B=[0, 2 ** 20], H=[0], Cin=[16, 32, 96], Cout=[0, 72], ks=[2, 5], stride=[0])
        e["dims"] = dict(Cin=axes["Cin"], Cout=axes["Cout"], ks=axes["ks"])
    base.update(e.get("base", {}))
    for a, k in e["args"]:
        if k == "p":
            axes[a] = PTR_VALUES
            bad[a] = PTR_VALUES[1:]
    for a in e.get("int8", ()):
        axes[a] = [0.0, 1.0, -1.0, math.nan]
        bad[a] = [0.0]
    for a in ("res_dtype", "out_dtype", "a_dtype"):
        if a in kinds:
            axes[a] = [F16, I8, F32]
            bad[a] = [I8, F32]
    if "relu" in kinds:
        axes["relu"] = [0, 1]
    if e.get("tables"):
        axes["dst"] = sorted(DST_TABLES) + ["NULL"]
        axes["ndst"] = [None, -1, 0, 1, 9]
        bad["dst"] = [t for t in axes["dst"] if t not in ("ok1", "ok2", "ok2_res", "eight")]
        bad["ndst"] = [0, 9]
    axes.update(e.get("axes", {}))
    bad.update(e.get("bad", {}))
    dims = e.get("dims")
    if dims is None:
        dims = {a: v for a, v in (("m", M_VALUES), ("n", N_VALUES), ("k", K_VALUES)) if a in kinds}
    for a, v in BAD_DIMS.items():
        if a in kinds:
            bad.setdefault(a, v)
    e.update(base=base, axes=axes, dims=dims, bad=bad)
    return e


def tuples(e):
    """the entry's grid as {label: tuple}: the base, the full product of its dims, every axis value alone, every pair of
    bad picks of two different arguments, and for the int8 flavours the product of scales, dtype codes and an identity
    present or absent"""
    base, out = e["base"], {}

    def add(**change):
        t = dict(base, **change)
        label = " ".join(f"{a}={t[a]}" for a, _ in e["args"] if a in t and t[a] != base[a])
        out.setdefault(label or "base", t)

    add()
    names = list(e["dims"])
    for combo in itertools.product(*(e["dims"][a] for a in names)):
        add(**dict(zip(names, combo)))
    for a, values in e["axes"].items():
        for v in values:
            add(**{a: v})
    picks = [(a, v) for a, values in e["bad"].items() for v in values]
    for (a, va), (b, vb) in itertools.combinations(picks, 2):
        if a != b:
            add(**{a: va, b: vb})
    if "int8" in e:
        kinds = dict(e["args"])
        sw = [a for a in e["int8"]] + [a for a in ("a_dtype", "res_dtype", "out_dtype") if a in kinds] + ["wsc", "res"]
        values = [[0.0, 1.0] if kinds[a] == "f" else ["A", "NULL"] if kinds[a] == "p" else [F16, I8, F32] for a in sw]
        for combo in itertools.product(*values):
            add(**dict(zip(sw, combo)))
    return out


def call(fn, e, t):
    args, slot, nk_sum = [], 0, 0
    for a, k in e["args"]:
        v = t[a]
        if k == "p":
            args.append(ptr(slot, v))
            slot += 1
        elif k == "stream":
            args.append(None)
        elif k == "dst":
            tab, n = dst_table(v, t["ndst"])
            args += [ctypes.cast(tab, P) if tab is not None else None, n]
        elif k == "ndst":
            pass
        elif k == "shapes":
            arr, nk_sum = shapes_array(v)
            args.append(ctypes.cast(arr, P) if arr is not None else None)
            t = dict(t, _keep=arr)
        elif k == "gstride":
            args.append(t["m"] * 256 + {"equal": 0, "below": -8, "unaligned": 4, "above": 256}[v])
        elif k == "nk":
            args.append({"sum": nk_sum, "sum-1": nk_sum - 1, "zero": 0}[v])
        elif k == "pbytes":
            arr, nk_sum2 = shapes_array(t["shapes"])
            size = 0
            if arr is not None:
                nk = {"sum": nk_sum2, "sum-1": nk_sum2 - 1, "zero": 0}[t["nk"]]
                size = t["_size"](ctypes.cast(arr, P), t["cams"], nk, t["heads"], t["ch"], t["levels"], t["nq"], t["np"])
            args.append({"size": size, "size-1": max(size - 1, 0), "zero": 0}[v])
        else:
            args.append(v)
    return fn(*args)


CTYPES = dict(p=P, stream=P, dst=P, ndst=I, shapes=P, gstride=LL, nk=I, pbytes=SZ, ll=LL, i=I, f=F, sz=SZ)


def bind(lib, name):
    fn = getattr(lib, name)
    fn.restype = ENTRIES[name].get("restype", I)
    fn.argtypes = [CTYPES[k] for _, k in ENTRIES[name]["args"]]
    return fn


def statuses(lib_path, name, labels=None):
    """(label, status) of the entry's grid, or of the listed labels of it"""
    lib = ctypes.CDLL(lib_path)
    e = spec(name)
    fn = bind(lib, name)
    extra = {}
    if name == "bevops_value_proj_packed":
        extra["_size"] = bind(lib, "bevops_value_proj_packed_size")
    grid = tuples(e)
    for label in (grid if labels is None else labels):
        yield label, call(fn, e, dict(grid[label], **extra))


def check(lib_path, golden_path):
    """compare the library against recorded statuses ({entry: {label: status}}, tests/golden/gemm_status.json)"""
    import json
    bad = total = 0
    for short, want in json.load(open(golden_path)).items():
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
        print("gemm_status_sweep.py passes host pointers: it must not run where a kernel could launch")
        return 3
    lib_path = sys.argv[1]
    if len(sys.argv) > 3 and sys.argv[2] == "--check":
        return check(lib_path, sys.argv[3])
    if len(sys.argv) > 3 and sys.argv[2] == "--entry":
        for label, status in statuses(lib_path, sys.argv[3]):
            print(f"{sys.argv[3][len('bevops_'):]}  {label}  -> {status}")
        return 0
    total, failed, digest = 0, 0, "--digest" in sys.argv[2:]
    for name in ENTRIES:
        r = subprocess.run([sys.executable, __file__, lib_path, "--entry", name], capture_output=True, text=True)
        if digest:      # the entry's lines as their count per status and one hash: what is kept under profiles/
            counts = collections.Counter(line.rsplit(" ", 1)[1] for line in r.stdout.splitlines())
            print(name[len("bevops_"):], " ".join(f"status{k}:{v}" for k, v in sorted(counts.items())),
                  "sha256:" + hashlib.sha256(r.stdout.encode()).hexdigest())
        else:
            sys.stdout.write(r.stdout)
        total += r.stdout.count("\n")
        if r.returncode != 0:
            failed += 1
            print(f"{name[len('bevops_'):]}  CHILD EXIT {r.returncode}")
            sys.stderr.write(r.stderr[-2000:])
    print(f"# {total} tuples, {len(ENTRIES)} entries")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
