"""CPU-only: the preconditions of tests/util_int8_ln.py over every case test_tsgemm_s8_ln_gpu.py runs, its tolerance on an
fp32 emulation of the norm, and the argument checks of bevops_tsgemm_s8_ln that return before any device call."""
import ctypes

import numpy as np
import pytest

import util_exact_dense as X
import util_int8_ln as U

CUS = 256      # MI355X; the GPU test computes its large row counts from the device it runs on


@pytest.fixture(scope="module")
def evaluated():
    """case id -> (case, pre-norm binary16 bits, ln_weight, ln_bias, float64 reference), computed once."""
    out = {}
    for c in U.cases(CUS):
        pre = U.pre_norm(c, X.make_ops(c))            # BudgetError here = the operands left the exact budget
        g, b = U.ln_params(c)
        out[c["id"]] = (c, pre, g, b, U.reference(pre, g, b))
    return out


def test_cases_cover_the_kernel():
    small = U.small_cases()
    assert {(c["M"], c["K"]) for c in small} == {(m, k) for m in (1, 31, 33, 160) for k in (128, 256, 384, 512)}
    everything = U.cases(CUS)
    assert len({c["id"] for c in everything}) == len(everything)
    assert all(c["N"] == 256 and not c["relu"] and c["out"] == "fp16" and c["mode"] == X.S8 for c in everything)
    # the flags cycle with co-prime periods: every value of each meets every value of the others
    seen = {(c["bias"], c["per_channel"], c["res"]) for c in small}
    assert {s[0] for s in seen} == {True, False} and {s[1] for s in seen} == {True, False}
    assert {s[2] for s in seen} == {None, "fp16", "int8"}
    assert {(s[1], s[2]) for s in seen} == {(p, r) for p in (True, False) for r in (None, "fp16", "int8")}
    assert {(s[0], s[2]) for s in seen} == {(p, r) for p in (True, False) for r in (None, "fp16", "int8")}
    # the large cases: the partition the exact test of tsgemm_s8 pins, identity kinds all present
    large = [U.large_case(j, CUS) for j in range(X.TS_LARGE)]
    assert [X.ts_block_passes(c["M"], CUS) for c in large] == X.ts_expected_partition(CUS)
    assert {c["res"] for c in large} == {None, "fp16", "int8"} and all(c["M"] % 32 == 17 and c["K"] == 128 for c in large)


def test_preconditions(evaluated):
    """Inside the exact budget (no BudgetError while building `evaluated`), no constant row, the stated parameters."""
    for cid, (c, pre, g, b, want) in evaluated.items():
        assert pre.shape == (c["M"], 256) and np.isfinite(pre.astype(np.float64)).all(), cid
        assert (pre.astype(np.float64).std(axis=1) > 0).all(), f"{cid}: a row with zero variance"
        r = X._rng("ln", cid)
        assert np.array_equal(g, (1.0 + 0.2 * r.standard_normal(256)).astype(np.float16)), cid
        assert np.array_equal(b, (0.1 * r.standard_normal(256)).astype(np.float16)), cid
        assert g.dtype == b.dtype == np.float16 and np.isfinite(want).all()


@pytest.mark.parametrize("ulps", [-3, 0, 3])
def test_tolerance_holds_for_an_fp32_norm(evaluated, ulps):
    """The conditions the kernel is held to, on the fp32 emulation with rstd off by `ulps` fp32 ulps."""
    worst, share = 0.0, 0.0
    for cid, (c, pre, g, b, want) in evaluated.items():
        got = U.emulate_f32(pre, g, b, U.EPS, ulps)
        U.check(got, want, f"{cid} rstd {ulps:+d} ulps")
        w, s = U.measure(got, want)
        worst = max(worst, w)
        if c["M"] >= U.MISROUND_MIN_M:
            share = max(share, s)
    print(f"rstd {ulps:+d} ulps: worst {worst:.4f} of the tolerance, at most {100 * share:.4f} % mis-rounded")
    assert worst <= 0.75 and share <= U.MISROUND_CAP / 2      # the emulation stays well inside: the bounds have margin


def test_check_rejects_what_it_should(evaluated):
    c, pre, g, b, want = evaluated[U.small_cases()[7]["id"]]          # a 160-row case
    assert c["M"] == 160
    good = want.astype(np.float16)
    U.check(good, want, "correctly rounded")
    two_ulps = good.copy()
    two_ulps[5, 7] = np.nextafter(np.nextafter(good[5, 7], np.float16(np.inf)), np.float16(np.inf))
    with pytest.raises(AssertionError, match="beyond one binary16 ulp"):
        U.check(two_ulps, want, "two ulps")
    one_percent = good.copy()
    idx = np.arange(0, good.size, 100)
    flat = one_percent.reshape(-1)
    toward = np.where(want.reshape(-1)[idx] > flat[idx].astype(np.float64), np.inf, -np.inf).astype(np.float16)
    flat[idx] = np.nextafter(flat[idx], toward)                        # the other neighbour of the float64 value
    with pytest.raises(AssertionError, match="not the correctly rounded"):
        U.check(one_percent, want, "1 % one ulp off")
    stale = np.roll(good, 32, axis=0)                                  # rows of another unit: far outside
    with pytest.raises(AssertionError):
        U.check(stale, want, "rows of another unit")


def test_entry_rejects_bad_params_without_gpu():
    """bevops_tsgemm_s8_ln: 2 = BAD_PARAM, 3 = NOT_SUPPORTED, all before any device call."""
    from bevformer_tensorrt_amd.utils import load_library
    lib = load_library()
    f, ll = ctypes.c_float, ctypes.c_longlong
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(ln_w=p, ln_b=p, eps=1e-5, out=p, n=256, k=128, a=p, s_a=0.05, res=None, res_dtype=1, s_res=1.0):
        return lib.bevops_tsgemm_s8_ln(a, f(s_a), p, None, f(0.01), None, res, res_dtype, f(s_res), ln_w, ln_b, f(eps), out,
                                       ll(64), n, k, None)
    assert call(ln_w=None) == 2                  # no norm weight
    assert call(ln_b=None) == 2                  # no norm bias
    assert call(eps=-1.0) == 2                   # negative eps
    assert call(eps=float("nan")) == 2           # !(eps >= 0)
    assert call(out=p + 8) == 2                  # misaligned out (fp16 rows: 16 bytes)
    assert call(ln_w=p + 8) == 2 and call(ln_b=p + 4) == 2
    assert call(n=512) == 3                      # N != 256
    assert call(k=192) == 3                      # K % 128
    assert call(a=None) == 2 and call(s_a=0.0) == 2            # as bevops_tsgemm_s8
    assert call(res=p, res_dtype=0) == 3                       # fp32 identity
    assert call(res=p, res_dtype=2, s_res=0.0) == 2            # int8 identity without a scale
    assert lib.bevops_query(b"bevops_tsgemm_s8_ln") == ctypes.cast(lib.bevops_tsgemm_s8_ln, ctypes.c_void_p).value
