"""CPU-only: which implementation the dense / convolution dispatch picks (functions/dispatch.py).
tests/golden/dispatch_choice.json holds what dense_auto and conv3x3_auto answered BEFORE the policy moved into
functions/dispatch.py -- every problem of the shipped table and a grid across every threshold of the rules, under every
combination of DETERMINISTIC / OWN_KERNELS / stream capture / BEVOPS_DENSE_TUNE / HALO, plus the edges (empty inputs, the
NOT_SUPPORTED fall-back, measured once, per-thread flags): tools/dispatch_choice_sweep.py wrote it and explains the
tokens.  The two pure choice functions must give every recorded token, and the entry points, driven by the tool in a
child process that sees no device, must too."""
import importlib.util
import json
import os
import subprocess
import sys

from conftest import GOLDEN, ROOT

RECORDED = os.path.join(GOLDEN, "dispatch_choice.json")
EDGES = ["dense M == 0", "conv B == 0, Cin % 32 == 0", "dense: tsgemm answers NOT_SUPPORTED", "dense: tsgemm answers BAD_PARAM",
         "dense: tsgemm answers FAILURE", "dense: blaslt answers NOT_SUPPORTED", "conv: tile answers NOT_SUPPORTED",
         "dense: an unseen problem posed twice", "conv: an unseen problem posed twice",
         "dense: the measurement, small answers NOT_SUPPORTED", "dense: the measurement, tile answers FAILURE",
         "conv: the measurement", "flags set on this thread: this thread / another thread"]


def _tool():
    spec = importlib.util.spec_from_file_location("dispatch_choice_sweep", os.path.join(ROOT, "tools", "dispatch_choice_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_recording_covers_what_it_must():
    S = _tool()
    assert os.path.getsize(RECORDED) < (1 << 20)
    table = S.load(RECORDED)
    flat = S.cases(table)
    assert len(flat) > 40000
    names = {family: {tok.split("+")[0] for case, tok in flat.items() if case.startswith(family)} for family in ("dense", "conv")}
    assert names["dense"] == {"tsgemm", "tile", "small", "blaslt", "torch", "measure"}
    assert names["conv"] == {"tile", "halo", "library", "measure[tile|library]", "measure[tile|library|halo]"}
    for tune in S.TUNES:
        assert sorted(table["edges"][tune]) == sorted(EDGES), tune
    e = table["edges"]["unset"]
    assert e["dense M == 0"] == "empty[0,256]" and e["conv B == 0, Cin % 32 == 0"] == "tile"        # (no +c, no +m)
    assert e["dense: tsgemm answers NOT_SUPPORTED"] == "fallback"
    assert e["dense: blaslt answers NOT_SUPPORTED"] == "raises status 3"
    assert e["dense: tsgemm answers BAD_PARAM"] == "raises status 2" and e["dense: tsgemm answers FAILURE"] == "raises status 1"
    assert e["dense: an unseen problem posed twice"] == {"first": "measure+c+m", "second": "tsgemm+c+m"}
    assert e["conv: an unseen problem posed twice"] == {"first": "measure[tile|library|halo]+c+m", "second": "tile+c+m"}
    assert e["flags set on this thread: this thread / another thread"] == ["tsgemm", "torch+c"]
    assert [m[1:] for m in e["dense: the measurement, small answers NOT_SUPPORTED"]["timed (candidate, iters, rounds)"]] == [[8, 3]] * 4
    assert [m[1:] for m in e["conv: the measurement"]["timed (candidate, iters, rounds)"]] == [[4, 3]] * 3
    # the shipped table's problems, BEVOPS_DENSE_TUNE unset, not capturing: every one listed, none missed
    assert S.counts(table) == {
        "dense table": {"blaslt+c": 51, "torch+c": 15, "tile+c": 14, "tsgemm+c": 7, "small+c": 6},
        "dense own": {"tile": 43, "tsgemm": 31, "small": 19},
        "dense rule": {"tsgemm": 47, "tile": 32, "small": 14}, "dense rule+own": {"tsgemm": 47, "tile": 32, "small": 14},
        "conv table": {"tile+c": 24, "library+c": 13, "halo+c": 5}, "conv own": {"tile+c": 24, "library+c": 13, "halo+c": 5},
        "conv rule": {"tile": 37, "halo": 5}, "conv rule+own": {"tile": 37, "halo": 5}}


def test_pure_choices_give_every_recorded_token():
    from bevformer_tensorrt_amd.functions import dispatch as D
    S = _tool()
    recorded = S.load(RECORDED)
    shipped = json.load(open(os.path.join(ROOT, "bevformer_tensorrt_amd", "dispatch_gfx950.json")))
    loaded = {"dense": shipped["dense"], "conv": shipped["conv"], "measured_dense": shipped["measured_us"]["dense"]}
    empty = {"dense": {}, "conv": {}, "measured_dense": {}}          # (BEVOPS_DENSE_TUNE = 0 / 1: the table is not loaded)
    contexts = [(rule, own, cap) for _, rule, own in S.MODES for cap in (False, True)]
    wrong, n = [], 0

    def token(name, keep, miss, timed=""):
        return name + (timed if name == "measure" else "") + ("+c" if keep else "") + ("+m" if miss else "")

    for tune in S.TUNES:
        table, value = (loaded if tune == "unset" else empty), ("" if tune == "unset" else tune)
        for prob, text in recorded["dense"][tune].items():
            M, N, K, relu, has_b, has_r = (int(v) for v in prob.split(","))
            key = ("meta", M, N, K, bool(relu), bool(has_b), bool(has_r))
            for (rule, own, cap), want in zip(contexts, S.unpack(text)):
                got = token(*D.dense_choice(key, rule, own, cap, value, table))
                n += 1
                if got != want:
                    wrong.append((tune, "dense", prob, rule, own, cap, want, got))
        for halo, problems in recorded["conv"][tune].items():
            for prob, text in problems.items():
                v = [int(x) for x in prob.split(",")]
                if v[0] == 0 and v[3] % 32 == 0:
                    continue        # (conv3x3_auto answers an empty batch before it chooses: the child-process test)
                key = ("meta", *v[:7], bool(v[7]), bool(v[8]))
                timed = "[tile|library|halo]" if D.halo_ok(key, halo == "halo") else "[tile|library]"
                for (rule, own, cap), want in zip(contexts, S.unpack(text)):
                    got = token(*D.conv_choice(key, rule, cap, value, table, halo == "halo"), timed)
                    n += 1
                    if got != want:
                        wrong.append((tune, "conv " + halo, prob, rule, own, cap, want, got))
    assert not wrong, (len(wrong), wrong[:10])
    assert n > 40000
    # what the process cache holds answers before the table does, except in the modes that never ask it
    key = ("meta", 40000, 256, 256, False, True, False)
    assert D.dense_choice(key, False, False, False, "", loaded, "tile") == ("tile", False, False)
    assert D.dense_choice(key, True, False, False, "", loaded, "tile") == ("tsgemm", False, False)
    assert D.dense_choice(key, False, False, lambda: True, lambda: "", empty) == ("tsgemm", False, True)     # asked lazily


def test_using_sets_and_restores_the_flags():
    from bevformer_tensorrt_amd.functions import dispatch as D, linear as L
    assert L.DETERMINISTIC is D.DETERMINISTIC and L.OWN_KERNELS is D.OWN_KERNELS
    L.OWN_KERNELS["enabled"] = True
    try:
        with D.using(rule=True):
            assert D.DETERMINISTIC["enabled"] is True and D.OWN_KERNELS["enabled"] is True
            with D.using(rule=False, own=False):
                assert D.DETERMINISTIC["enabled"] is False and D.OWN_KERNELS["enabled"] is False
            assert D.DETERMINISTIC["enabled"] is True and D.OWN_KERNELS["enabled"] is True
        assert D.DETERMINISTIC["enabled"] is False and D.OWN_KERNELS["enabled"] is True
        try:
            with D.using(own=False):
                raise KeyError("inside")
        except KeyError:
            pass
        assert D.OWN_KERNELS["enabled"] is True
    finally:
        L.OWN_KERNELS["enabled"] = False


def test_entry_points_give_every_recorded_token():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) +
                       [os.path.join(ROOT, "tools", "dispatch_choice_sweep.py"), "--check", RECORDED],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, f"{r.stdout[-4000:]}\n{r.stderr[-2000:]}"
    assert "recorded cases, 0 differ" in r.stdout
