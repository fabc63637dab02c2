#!/usr/bin/env python3
"""Which implementation dense_auto (functions/linear.py) and conv3x3_auto (functions/conv.py) run, as text: calls the two
entry points on `meta` tensors -- every problem of the shipped table, a grid that straddles every threshold of the rules,
under every combination of DETERMINISTIC / OWN_KERNELS / stream capture / BEVOPS_DENSE_TUNE / HALO -- with the candidates
replaced by stubs that return their own name, and writes per case: the candidate that ran (or `measure` with the candidates
that would be timed), whether the choice is in the process cache afterwards (`+c`) and whether the problem went to the miss
list (`+m`).  tests/golden/dispatch_choice.json holds what the code answered BEFORE the policy moved to
functions/dispatch.py; tests/test_dispatch_choice_cpu.py compares.  The file is grouped by outcome (`store` / `load`):
every problem is named in it, next to the tokens it gave under BEVOPS_DENSE_TUNE unset / 0 / 1.

No kernel runs: the sweep works in child processes that see no device, one per value of BEVOPS_DENSE_TUNE (the shipped
table is loaded once per process).

usage: dispatch_choice_sweep.py --record OUT.json | --check RECORDED.json | --counts"""
import collections
import contextlib
import itertools
import json
import os
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNES = ("unset", "0", "1")
MODES = (("table", False, False), ("own", False, True), ("rule", True, False), ("rule+own", True, True))
CONTEXTS = [name + cap for name, _, _ in MODES for cap in ("", "/capture")]      # one token per context, in this order
DENSE_GRID = ([1, 63, 64, 900, 2048, 2049, 8193, 40000], [8, 72, 192, 256, 512, 2048], [4, 8, 64, 192, 200, 256, 1024, 1088],
              [(0, 1, 0), (1, 1, 0), (0, 1, 1), (0, 0, 0)])                       # M, N, K, (relu, bias, residual)
CONV_GRID = ([0, 1, 6], [3, 16, 32, 64, 128], [64, 128], [1, 2], [0, 1])           # B, Cin, Cout, stride, residual
CONV_HW = (12, 20)                                                                 # (no model poses this image size)


def pack(tokens):
    """['a', 'a', 'b'] -> 'a*2 b'"""
    return " ".join(t if n == 1 else f"{t}*{n}" for t, n in ((t, len(list(g))) for t, g in itertools.groupby(tokens)))


def unpack(text):
    out = []
    for part in text.split(" "):
        tok, _, n = part.partition("*")
        out += [tok] * int(n or 1)
    return out


def sweep():
    """The child's work: every case under this process's BEVOPS_DENSE_TUNE -> {"dense": ..., "conv": ..., "edges": ...}"""
    import torch
    assert not torch.cuda.is_available(), "the sweep stubs the device away: run it where torch sees none"
    sys.path.insert(0, ROOT)
    from bevformer_tensorrt_amd.functions import conv as C, linear as L
    from bevformer_tensorrt_amd.utils import lib as _lib
    capturing, measured = {"on": False}, []
    torch.cuda.is_current_stream_capturing = lambda: capturing["on"]
    torch.cuda.synchronize = lambda *a, **k: None
    torch.cuda.device = lambda *a, **k: contextlib.nullcontext()

    def named(name):
        return lambda *a, **k: name

    real_dense, real_lba, real_measure = dict(L._DENSE), L.linear_bias_act, L._dense_measure
    for n in real_dense:
        L._DENSE[n] = named(n)
    L.linear_bias_act = named("fallback")
    conv_stubs = C._CONV                                          # (the candidate table of conv3x3_auto)
    for n in ("tile", "halo", "library"):
        conv_stubs[n] = named(n)

    def fake_dense_measure(key, *a, **k):
        measured.append(list(L._DENSE))
        return next(iter(L._DENSE))

    def fake_time(fn, iters=8, rounds=3):
        measured.append((fn(), iters, rounds))
        return float(len(measured))

    L._dense_measure = fake_dense_measure
    for mod in {sys.modules[getattr(L, n).__module__] for n in ("graph_time_us", "_table")} | {L, C}:
        if hasattr(mod, "graph_time_us"):
            mod.graph_time_us = fake_time

    def reset():
        for box in (L._DENSE_CHOICE, L.DENSE_MISSES, L.DENSE_LOG, C._CHOICE, C.CONV_MISSES, C.CONV_LOG, measured):
            box.clear()

    def token(ran, cached, miss):
        if measured:
            ran = "measure" if isinstance(measured[0], list) else "measure[" + "|".join(m[0] for m in measured) + "]"
        return ran + ("+c" if cached else "") + ("+m" if miss else "")

    def dense(M, N, K, relu, has_b, has_r, fresh=True):
        if fresh:
            reset()
        x, w = torch.empty(M, K, dtype=torch.float16, device="meta"), torch.empty(N, K, dtype=torch.float16, device="meta")
        b = torch.empty(N, dtype=torch.float16, device="meta") if has_b else None
        r = torch.empty(M, N, dtype=torch.float16, device="meta") if has_r else None
        ran = L.dense_auto(x, w, b, r, bool(relu))
        if not isinstance(ran, str):
            ran = "empty" + str(list(ran.shape)).replace(" ", "")
        key = (str(x.device), M, N, K, bool(relu), bool(has_b), bool(has_r))
        return token(ran, key in L._DENSE_CHOICE, L._problem(key) in L.DENSE_MISSES)

    def conv(Bn, H, W, Cin, Cout, k, stride, relu, has_r, fresh=True):
        if fresh:
            reset()
        x = torch.empty(Bn, Cin, H, W, dtype=torch.float16, device="meta")
        w = torch.empty(Cout, Cin, k, k, dtype=torch.float16, device="meta")
        Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
        r = torch.empty(Bn, Cout, Ho, Wo, dtype=torch.float16, device="meta") if has_r else None
        ran = C.conv3x3_auto(x, w, None, bool(relu), r, stride)
        key = (str(x.device), Bn, H, W, Cin, Cout, k, stride, bool(relu), bool(has_r))
        return token(ran, key in C._CHOICE, L._problem(key) in C.CONV_MISSES)

    def contexts(case, *problem):
        out = []
        for _, rule, own in MODES:
            for cap in (False, True):
                L.DETERMINISTIC["enabled"], L.OWN_KERNELS["enabled"], capturing["on"] = rule, own, cap
                out.append(case(*problem))
        L.DETERMINISTIC["enabled"] = L.OWN_KERNELS["enabled"] = capturing["on"] = False
        return pack(out)

    shipped = json.load(open(os.path.join(ROOT, "bevformer_tensorrt_amd", "dispatch_gfx950.json")))
    res = {"dense": {}, "conv": {"halo": {}, "nohalo": {}}}
    problems = [tuple(int(v) for v in p.split(",")) for p in sorted(shipped["dense"])]
    problems += [(M, N, K) + e for M, N, K, e in itertools.product(*DENSE_GRID)]
    for p in problems:
        res["dense"][",".join(map(str, p))] = contexts(dense, *p)
    problems = [tuple(int(v) for v in p.split(",")) for p in sorted(shipped["conv"])]
    problems += [(Bn,) + CONV_HW + (Cin, Cout, 3, s, 1, r) for Bn, Cin, Cout, s, r in itertools.product(*CONV_GRID)]
    was = C.HALO["enabled"]
    for halo in ("halo", "nohalo"):
        C.HALO["enabled"] = halo == "halo"
        for p in problems:
            res["conv"][halo][",".join(map(str, p))] = contexts(conv, *p)
    C.HALO["enabled"] = was

    # ---- the edges (not capturing, both flags off unless stated) -------------------------------------------------
    edges = {}
    edges["dense M == 0"] = dense(0, 256, 256, 0, 1, 0)
    edges["conv B == 0, Cin % 32 == 0"] = conv(0, 12, 20, 64, 64, 3, 1, 1, 0)

    def raising(status):
        def fn(*a, **k):
            raise _lib.BevopsError("stub", status)
        return fn

    def outcome(fn):
        try:
            return fn()
        except _lib.BevopsError as exc:
            return "raises status %d" % exc.status

    L.DETERMINISTIC["enabled"] = True                       # 40000 x 256 x 256 by rule: tsgemm; 900 x 72 x 200: tile
    for name, status in (("NOT_SUPPORTED", _lib.NOT_SUPPORTED), ("BAD_PARAM", _lib.BAD_PARAM), ("FAILURE", _lib.FAILURE)):
        L._DENSE["tsgemm"] = raising(status)
        edges["dense: tsgemm answers " + name] = outcome(lambda: dense(40000, 256, 256, 0, 1, 0))
    L._DENSE["tsgemm"] = named("tsgemm")
    L.DETERMINISTIC["enabled"] = False
    L._DENSE["blaslt"] = raising(_lib.NOT_SUPPORTED)        # 63 rows, K % 64 != 0: the default, blaslt
    edges["dense: blaslt answers NOT_SUPPORTED"] = outcome(lambda: dense(63, 72, 200, 0, 1, 0))
    L._DENSE["blaslt"] = named("blaslt")
    conv_stubs["tile"] = raising(_lib.NOT_SUPPORTED)
    L.DETERMINISTIC["enabled"] = True
    edges["conv: tile answers NOT_SUPPORTED"] = outcome(lambda: conv(1, 12, 20, 128, 128, 3, 1, 1, 0))
    L.DETERMINISTIC["enabled"] = False
    conv_stubs["tile"] = named("tile")

    def twice(case, *problem):
        first = case(*problem)
        measured.clear()
        second = case(*problem, fresh=False)          # (the caches as the first call left them)
        return {"first": first, "second": second}

    edges["dense: an unseen problem posed twice"] = twice(dense, 2049, 72, 200, 0, 1, 0)
    edges["conv: an unseen problem posed twice"] = twice(conv, 1, 12, 20, 64, 64, 3, 1, 1, 0)

    # the measurement itself: the real _dense_measure over the stubs, with `small` outside its domain
    reset()
    L._dense_measure = real_measure
    L._DENSE["small"] = raising(_lib.NOT_SUPPORTED)
    x, w = torch.empty(2049, 200, dtype=torch.float16, device="meta"), torch.empty(72, 200, dtype=torch.float16, device="meta")
    ran = L.dense_auto(x, w, None, None, False)
    edges["dense: the measurement, small answers NOT_SUPPORTED"] = {
        "ran": ran, "timed (candidate, iters, rounds)": [list(m) for m in measured], "log": [[list(k), t] for k, t in L.DENSE_LOG]}
    L._DENSE["tile"] = raising(_lib.FAILURE)
    reset()
    edges["dense: the measurement, tile answers FAILURE"] = outcome(lambda: L.dense_auto(x, w, None, None, False))
    L._DENSE["small"], L._DENSE["tile"], L._dense_measure = named("small"), named("tile"), fake_dense_measure
    reset()
    conv(6, 12, 20, 64, 64, 3, 1, 1, 0)
    edges["conv: the measurement"] = {"timed (candidate, iters, rounds)": [list(m) for m in measured],
                                     "log": [[list(k), t] for k, t in C.CONV_LOG]}

    # the per-thread flags: set here, a table problem posed on another thread takes the table's choice
    seen = []
    L.DETERMINISTIC["enabled"] = L.OWN_KERNELS["enabled"] = True
    here = dense(40000, 256, 256, 0, 1, 0)
    t = threading.Thread(target=lambda: seen.append(dense(40000, 256, 256, 0, 1, 0)))
    t.start()
    t.join()
    L.DETERMINISTIC["enabled"] = L.OWN_KERNELS["enabled"] = False
    edges["flags set on this thread: this thread / another thread"] = [here, seen[0]]
    res["edges"] = edges
    L._DENSE.update(real_dense)
    L.linear_bias_act = real_lba
    return res


def run_all():
    out = {"contexts": CONTEXTS, "tokens": "candidate that ran, or measure / measure[candidates timed]; +c: the choice is in "
           "the process cache afterwards; +m: the problem went to the miss list; tok*n: n contexts in a row",
           "dense": {}, "conv": {}, "edges": {}}
    children = {}
    for tune in TUNES:
        env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
        env.pop("BEVOPS_DENSE_TUNE", None)
        if tune != "unset":
            env["BEVOPS_DENSE_TUNE"] = tune
        children[tune] = subprocess.Popen([sys.executable] + (["-s"] if sys.flags.no_user_site else []) +
                                          [os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, text=True,
                                          stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    for tune, child in children.items():
        stdout, stderr = child.communicate()
        if child.returncode != 0:
            sys.exit(f"BEVOPS_DENSE_TUNE {tune}: the sweep failed\n{stdout[-2000:]}\n{stderr[-4000:]}")
        got = json.loads(stdout.splitlines()[-1])
        for family in ("dense", "conv", "edges"):
            out[family][tune] = got[family]
    return out


def _outcome(table, family, prob):
    """a problem's tokens under every tune value (conv: with HALO ; without), as one string"""
    if family == "dense":
        return " / ".join(table["dense"][tune][prob] for tune in TUNES)
    return " / ".join(table["conv"][tune]["halo"][prob] + " ; " + table["conv"][tune]["nohalo"][prob] for tune in TUNES)


def store(table, path):
    """Writes a recording grouped by outcome: per family {tokens of unset / 0 / 1: the problems that gave them}, problems
    that differ in their first number only (M, B) written once with the numbers joined by `|`; one group per line."""
    lines = ['"contexts": ' + json.dumps(table["contexts"]), '"tokens": ' + json.dumps(table["tokens"])]
    for family in ("dense", "conv"):
        groups = collections.defaultdict(lambda: collections.defaultdict(list))
        problems = table[family]["unset"] if family == "dense" else table["conv"]["unset"]["halo"]
        for prob in sorted(problems, key=lambda p: [int(v) for v in p.split(",")][1:] + [int(p.split(",")[0])]):
            first, rest = prob.split(",", 1)
            groups[_outcome(table, family, prob)][rest].append(first)
        rows = [json.dumps(o) + ": " + json.dumps(" ".join("|".join(firsts) + "," + rest for rest, firsts in g.items()))
                for o, g in sorted(groups.items())]
        lines.append(f'"{family}": {{\n' + ",\n".join(rows) + "\n}")
    rows = [json.dumps(tune) + ": {\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, sort_keys=True)
                                                     for k, v in sorted(table["edges"][tune].items())) + "\n}" for tune in TUNES]
    lines.append('"edges": {\n' + ",\n".join(rows) + "\n}")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")


def load(path):
    """store's file as run_all returns it: table[family][tune]([halo])[problem] = packed tokens"""
    stored = json.load(open(path))
    table = dict(stored, dense={t: {} for t in TUNES}, conv={t: {"halo": {}, "nohalo": {}} for t in TUNES})
    for family in ("dense", "conv"):
        for outcome, problems in stored[family].items():
            for entry in problems.split(" "):
                firsts, rest = entry.split(",", 1)
                for first in firsts.split("|"):
                    for tune, text in zip(TUNES, outcome.split(" / ")):
                        if family == "dense":
                            table["dense"][tune][first + "," + rest] = text
                        else:
                            table["conv"][tune]["halo"][first + "," + rest], table["conv"][tune]["nohalo"][first + "," + rest] = text.split(" ; ")
    return table


def cases(table):
    """{case name: token} of a whole recording"""
    flat = {}
    for tune in TUNES:
        groups = [("dense", table["dense"][tune])] + [("conv " + h, t) for h, t in table["conv"][tune].items()]
        for family, problems in groups:
            for prob, text in problems.items():
                for ctx, tok in zip(CONTEXTS, unpack(text)):
                    flat[f"{family} {prob} tune={tune} {ctx}"] = tok
        for name, what in table["edges"][tune].items():
            flat[f"edge tune={tune} {name}"] = json.dumps(what, sort_keys=True)
    return flat


def counts(table):
    """candidate counts over the SHIPPED table's problems (BEVOPS_DENSE_TUNE unset, not capturing), per family and mode"""
    shipped = json.load(open(os.path.join(ROOT, "bevformer_tensorrt_amd", "dispatch_gfx950.json")))
    out = {}
    for family, problems in (("dense", table["dense"]["unset"]), ("conv", table["conv"]["unset"]["halo"])):
        for i, ctx in enumerate(CONTEXTS):
            if "/capture" not in ctx:
                c = collections.Counter(unpack(problems[p])[i] for p in shipped[family])
                out[f"{family} {ctx}"] = dict(sorted(c.items(), key=lambda kv: -kv[1]))
    return out


def main():
    if sys.argv[1:] == ["--child"]:
        print(json.dumps(sweep()))
    elif sys.argv[1:2] == ["--record"] and len(sys.argv) == 3:
        table = run_all()
        store(table, sys.argv[2])
        print(json.dumps(counts(table), indent=1))
        print(f"{len(cases(table))} cases recorded")
    elif sys.argv[1:2] == ["--check"] and len(sys.argv) == 3:
        want, got = cases(load(sys.argv[2])), cases(run_all())
        differ = [k for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)]
        for k in differ[:40]:
            print(f"{k}: recorded {want.get(k)}, now {got.get(k)}")
        print(f"{len(want)} recorded cases, {len(differ)} differ")
        sys.exit(1 if differ else 0)
    elif sys.argv[1:] == ["--counts"]:
        print(json.dumps(counts(run_all()), indent=1))
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
