"""tests/util_exact_dense.py checked without a GPU: the float64 references against naive Python loops, the operand
generators against the bit budget for every case the GPU files run, that those cases really exercise the final
rounding (inexact values, exact ties, saturation), and that they reach every tile_gemm_kernel instantiation and every
kloop<G> / two-pass partition of tsgemm_s8_kernel."""
import os
import re

import numpy as np
import pytest

import util_exact_dense as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rint_even(v):
    f = np.floor(v)
    d = v - f
    if d > 0.5 or (d == 0.5 and f % 2 == 1):
        return f + 1
    return f


def _naive(c, o):
    """The reference of a (tiny) case with Python loops and scalar float64 arithmetic."""
    a = X.ref_quantize(o["a"], o["s_a"]) if c["mode"] == X.F16Q else o["a"]
    a, w = a.astype(np.float64), o["w"].astype(np.float64)
    M, N = c["M"], c["N"]
    out = np.zeros((M, N), dtype=np.float16 if c["out"] == "fp16" else np.int8)
    for m in range(M):
        for n in range(N):
            acc = 0.0
            if c["conv"]:
                ho, wo = X.conv_out_hw(c["H"], c["W"], c["ks"], c["stride"])
                b, pix = divmod(m, ho * wo)
                yo, xo = divmod(pix, wo)
                for ty in range(c["ks"]):
                    for tx in range(c["ks"]):
                        y, x = yo * c["stride"] + ty - c["ks"] // 2, xo * c["stride"] + tx - c["ks"] // 2
                        if 0 <= y < c["H"] and 0 <= x < c["W"]:
                            for ci in range(c["Cin"]):
                                acc += a[b, y, x, ci] * w[n, ty, tx, ci]
            else:
                for k in range(c["K"]):
                    acc += a[m, k] * w[n, k]
            sw = o["s_w"] if np.isscalar(o["s_w"]) else float(o["s_w"][n])
            v = acc * (1.0 if c["mode"] == X.F16 else o["s_a"] * sw)
            if o["bias"] is not None:
                v += float(o["bias"][n])
            if o["res"] is not None:
                v += float(o["res"][m, n]) * (o["s_res"] if c["res"] == "int8" else 1.0)
            if c["relu"]:
                v = max(v, 0.0)
            if c["out"] == "fp16":
                out[m, n] = np.float16(v)           # float64 -> fp16 in one RNE step
            else:
                out[m, n] = int(min(max(_rint_even(v / o["s_out"]), -127), 127))
    return out


TINY = [X._case(mode=X.S8, M=3, N=5, K=16, bias=True, per_channel=True, relu=True, res="int8", out="int8", plant128=True),
        X._case(mode=X.S8, M=2, N=4, K=32, bias=True, res="fp16", out="fp16"),
        X._case(mode=X.F16Q, M=3, N=4, K=16, bias=True, per_channel=True, out="int8"),
        X._case(mode=X.F16Q, M=2, N=3, K=16, relu=True, res="fp16"),
        X._case(mode=X.F16, M=3, N=4, K=8, bias=True, res="fp16", relu=True),
        X._case(mode=X.S8, conv=True, B=2, H=3, W=2, Cin=64, Cout=3, ks=3, stride=2, bias=True, per_channel=True,
                relu=True, out="int8"),
        X._case(mode=X.F16, conv=True, B=1, H=2, W=3, Cin=32, Cout=2, ks=3, stride=1, bias=True, res="fp16"),
        X._case(mode=X.F16Q, conv=True, B=1, H=1, W=4, Cin=64, Cout=2, ks=1, stride=3, res="fp16")]


@pytest.mark.parametrize("c", TINY, ids=lambda c: c["id"])
def test_reference_is_the_naive_loop(c):
    o = X.make_ops(c)
    assert np.array_equal(X.reference(c, o), _naive(c, o))


def test_quantiser_reference_ties_and_clamps():
    x = (np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.5, 300.5, -127.5, -300.25, 3.25, -3.75]) * X.S_A)
    want = np.array([0, 2, 2, 0, -2, -2, 126, 127, 127, -127, -127, 3, -4], dtype=np.int8)
    assert np.array_equal(X.ref_quantize(x.astype(np.float16), X.S_A), want)
    assert np.array_equal([_rint_even(v) for v in x / X.S_A], np.rint(x / X.S_A))
    q = np.arange(-128, 128).astype(np.int8)
    assert np.array_equal(X.ref_dequantize(q, 2.0 ** -5).astype(np.float64), q.astype(np.float64) * 2.0 ** -5)
    acts = X.gen_f16q_acts(X._rng("t"), (64, 48)).astype(np.float64) / X.S_A
    assert (np.abs(acts - np.floor(acts) - 0.5) == 0).mean() > 0.2 and acts.max() > 127 and acts.min() < -127


def test_the_reference_raises_outside_the_budget():
    ok = np.array([[2.0 ** 24]])
    X.ref_epilogue(ok, 2.0 ** -11, None, None, False, "fp16")
    with pytest.raises(X.BudgetError, match="acc"):
        X.ref_epilogue(ok + 1, 2.0 ** -11, None, None, False, "fp16")
    with pytest.raises(X.BudgetError, match="bias"):
        X.ref_epilogue(ok, 1.0, np.array([0.5]), None, False, "fp16")
    with pytest.raises(X.BudgetError, match="identity"):
        X.ref_epilogue(ok, 1.0, None, np.array([[0.5]]), False, "fp16")
    with pytest.raises(X.BudgetError, match="scale"):
        X.ref_epilogue(np.array([[3.0]]), 2.0 ** -150, None, None, False, "fp16")
    # the saturated family: (float)acc is modelled as RNE (an odd integer above 2^24 is a tie and goes to the even
    # mantissa: 33 032 065 -> ...064, 33 032 067 -> ...068) and nothing else is relaxed
    got = X.ref_epilogue(np.array([[33032065.0, 33032067.0]]), 2.0 ** -11, None, None, False, "fp16", acc_rne=True)
    assert np.array_equal(got, (np.array([[33032064.0, 33032068.0]]) * 2.0 ** -11).astype(np.float16))
    with pytest.raises(X.BudgetError, match="bias"):
        X.ref_epilogue(np.array([[33032065.0]]), 1.0, np.array([0.5]), None, False, "fp16", acc_rne=True)


def _all_gpu_cases(cus=256):
    return X.gemm_cases() + X.conv_cases() + X.saturated_cases() + X.ts_cases(cus)


def test_every_gpu_case_is_inside_the_budget_and_exercises_the_rounding():
    """reference() raises BudgetError on any case outside the budget.  The shares are printed (run with -s)."""
    inexact = ties = count16 = 0
    tie8 = sat8 = count8 = 0
    per_family = {}
    for c in _all_gpu_cases():
        o = X.make_ops(c)
        acc, scale, bias, res = X.case_terms(c, o)
        ref = X.ref_epilogue(acc, scale, bias, res, c["relu"], c["out"], o["s_out"], acc_rne=c["sat"])
        assert ref.shape == (c["M"], c["N"])
        if c["sat"]:
            assert np.abs(acc).max() == 2048 * 127 * 127 and (np.abs(acc) > 2 ** 24).mean() > 0.9
            assert ((acc % 2 == 1) & (np.abs(acc) > 2 ** 24)).any()          # ties of the int -> float conversion
            acc = acc.astype(np.float32).astype(np.float64)
        v = X.exact_value(acc, scale, bias, res, c["relu"])
        fam = per_family.setdefault((c["mode"], c["conv"], c["out"]), [0, 0.0, 0.0])
        fam[0] += v.size
        if c["out"] == "fp16":
            assert np.isfinite(ref.astype(np.float64)).all()
            a, b = X.fp16_shares(v)
            inexact, ties, count16 = inexact + a * v.size, ties + b * v.size, count16 + v.size
        else:
            a, b = X.int8_shares(v / o["s_out"])
            tie8, sat8, count8 = tie8 + a * v.size, sat8 + b * v.size, count8 + v.size
            assert c["M"] * c["N"] < 4096 or c["sat"] or (a > 0 and b > 0), (c["id"], a, b)
        fam[1] += a * v.size
        fam[2] += b * v.size
    print(f"\nfp16-output cases: {count16} values, {inexact / count16:.4f} not fp16 numbers, {ties / count16:.5f} exact ties")
    print(f"int8-output cases: {count8} values, {tie8 / count8:.5f} ties of v / s_out, {sat8 / count8:.4f} beyond +-127")
    for (mode, conv, out), (n, a, b) in sorted(per_family.items()):
        print(f"  {mode:5s} conv={int(conv)} {out}: {n} values, {a / n:.5f} / {b / n:.5f}")
        assert a > 0 and b > 0, (mode, conv, out)


def test_gpu_cases_reach_every_tile_instantiation():
    src = open(os.path.join(ROOT, "bevformer_tensorrt_amd", "csrc", "tile_gemm.hip")).read()
    uses = re.findall(r"BEVOPS_TG\((true|false), (true|false), (true|false)\);", src)
    assert 2 * len(uses) == len(X.ALL_TILE_INSTANCES) == 22          # each use launches the narrow or the wide tile
    reached = {}
    for c in X.gemm_cases() + X.conv_cases() + X.saturated_cases():
        inst = X.case_instance(c)
        assert inst is not None, c["id"]
        reached.setdefault(inst, []).append(c["id"])
    for inst in sorted(X.ALL_TILE_INSTANCES):
        print(inst, len(reached.get(inst, ())))
    assert set(reached) == X.ALL_TILE_INSTANCES
    # where the launch code answers with a status instead
    assert X.tile_instance(X.F16Q, True, True, False, 64) is None and X.tile_instance(X.F16, False, True, False, 64) is None
    assert X.tile_instance(X.F16Q, False, False, True, 64) is None and X.tile_instance(X.S8, True, False, True, 64) is None


def test_every_flag_value_meets_the_edges():
    """Each value of each epilogue flag, per mode, runs with a ragged M, a ragged N (non-vector epilogue) and a K tail."""
    for mode, step in ((X.S8, 64), (X.F16Q, 64), (X.F16, 32)):
        cs = [c for c in X.gemm_cases() if c["mode"] == mode]
        assert {c["M"] for c in cs} >= set(X.GEMM_M) and {c["N"] for c in cs} >= set(X.GEMM_N)
        assert {c["K"] for c in cs} >= set(X.GEMM_K16 if mode == X.F16 else X.GEMM_K8)
        flags = {"bias": (False, True), "relu": (False, True), "res": (None, "fp16")}
        if mode != X.F16:
            flags.update(per_channel=(False, True), out=("fp16", "int8"))
        if mode == X.S8:
            flags["res"] = (None, "fp16", "int8")
        for name, values in flags.items():
            for val in values:
                sel = [c for c in cs if c[name] == val]
                assert any(c["M"] % 128 for c in sel), (mode, name, val, "ragged M")
                assert any(c["N"] % 8 for c in sel), (mode, name, val, "ragged N")
                assert any(c["N"] % 8 == 0 and c["N"] % 64 for c in sel), (mode, name, val, "vector path, ragged tile")
                assert any(c["K"] % step for c in sel), (mode, name, val, "K tail")
    M, N, _ = X.TILE_ORDER_SHAPE
    tiles = -(-M // 128) * -(-N // 128)
    assert tiles >= 9 and tiles % 8 != 0
    conv = X.conv_cases()
    for mode in (X.S8, X.F16Q, X.F16):
        cs = [c for c in conv if c["mode"] == mode]
        assert {(c["H"], c["W"], c["ks"], c["stride"]) for c in cs} == \
            {(h, w, k, s) for (h, w) in X.CONV_IMAGES for k in (1, 3) for s in (1, 2, 3)}
        assert {c["Cout"] for c in cs} == set(X.CONV_COUT) and len({c["Cin"] for c in cs}) == 2
        assert {c["res"] for c in cs} == {None, "fp16"}
    # a row tile that spans images (Hout * Wout not a multiple of 128, M > Hout * Wout) with int8 output and ReLU
    assert any(c["mode"] == X.S8 and c["out"] == "int8" and c["relu"] and (c["H"], c["W"]) == (7, 9) and c["stride"] == 1
               for c in conv)
    assert any(c["mode"] == X.S8 and c["out"] == "int8" and (c["H"], c["W"]) == (1, 1) for c in conv)


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_tsgemm_s8_row_counts_reach_every_unit_count(cus):
    ms = X.ts_large_m(cus)
    seen, two_pass = set(), False
    for M, want in zip(ms, X.ts_expected_partition(cus)):
        got = X.ts_block_passes(M, cus)
        print(cus, M, sorted(got))
        assert got == want and M % 32 != 0
        seen |= {p[0] for p in got if len(p) == 1}
        two_pass |= any(len(p) == 2 for p in got)
        passes = X.ts_s8_partition(M, cus)
        assert sum(g for _, g in passes) == -(-M // 32) and len({b for b, _ in passes}) == min(cus, -(-M // 32))
    assert seen == {1, 2, 3, 4, 5} and two_pass
    for M in X.TS_M_SMALL:
        assert X.ts_block_passes(M, cus) == {(1,)}
    assert X.ts_s8_partition(160, cus) == [(b, 1) for b in range(5)]
    # the mirror against the kernel's own words
    src = open(os.path.join(ROOT, "bevformer_tensorrt_amd", "csrc", "tsgemm.hip")).read()
    assert f"constexpr int kTsG = {X.TS_G};" in src
    cs = X.ts_cases(cus)
    assert {(c["N"], c["K"]) for c in cs} >= {(n, k) for n in X.TS_N for k in X.TS_K}
    assert {c["res"] for c in cs} == {None, "fp16", "int8"} and {c["out"] for c in cs} == {"fp16", "int8"}
    assert {c["per_channel"] for c in cs} == {False, True} and {c["relu"] for c in cs} == {False, True}
