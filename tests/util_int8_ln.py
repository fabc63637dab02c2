"""Cases, float64 reference and tolerance of the int8 GEMM with the LayerNorm in its epilogue (bevops_tsgemm_s8_ln,
tsgemm_s8_kernel<2> of csrc/tsgemm.hip).  Shared by test_int8_ln_cpu.py (which checks all of this without a GPU) and
test_tsgemm_s8_ln_gpu.py.

The kernel computes  out = LayerNorm_256(pre) * ln_weight + ln_bias  with  pre = fp16(acc * s_a * s_w[n] + bias[n]
(+ identity[m, n])).  On the dyadic operands of util_exact_dense.py every BIT of `pre` is predicted
(util_exact_dense.reference at tolerance 0), so the reference here is exact up to the normalisation: the LayerNorm of those
binary16 values evaluated in float64.

Tolerance.  The kernel normalises in fp32: mean = sum / 256, d = pre - mean, var = sum d^2 / 256, rstd = rsqrt(var + eps)
(an approximate instruction: a few fp32 ulps), y = fma(d * rstd, weight, bias), one rounding to binary16.  Its fp32 error
is some 2^-21 relative to |d * rstd * weight| + |bias| <= a few units, far below half a binary16 ulp (2^-15 at 2^-4), so
the result is the correctly rounded binary16 of the float64 value except where that value lies within the fp32 error of a
rounding boundary.  Hence the two conditions of `check`:
  * every output within ONE binary16 ulp of max(|want|, 2^-4) of the float64 value (a mis-rounding moves by at most one
    ulp at the value's own magnitude; 2^-4 is the floor below which the absolute fp32 error, not the ulp, is what counts);
  * in every case with M >= 31 at most 0.5 % of the outputs differ from the correctly rounded one.
test_int8_ln_cpu.py puts both on an fp32 emulation of the norm with rstd moved by +-3 fp32 ulps, over every case of the
GPU test (256 CUs): it reaches 0.503 of the first tolerance and mis-rounds at most 0.09 % of a case.  The share is not
capped at M = 1, where 2 of 256 outputs are already 0.78 %."""
import numpy as np

import util_exact_dense as X

N = 256
EPS = 1e-5
LN_K = X.TS_K                      # one step, two stages, the bi % nk rotation, the ring wrapping
LN_M_SMALL = X.TS_M_SMALL          # (1, 31, 33, 160)
MISROUND_CAP = 0.005
MISROUND_MIN_M = 31
ULP_FLOOR = 2.0 ** -4


def _ln_case(M, K, i):
    """Case i of a list: bias (period 2), identity kind (period 3) and per-channel scales (period 5) cycle with co-prime
    periods.  No ReLU, fp16 out: the flavour's domain."""
    return X._case(mode=X.S8, M=M, N=N, K=K, bias=i % 2 == 0, per_channel=i % 5 < 2, relu=False,
                   res=(None, "fp16", "int8")[i % 3], out="fp16")


def small_cases():
    cases, i = [], 0
    for K in LN_K:
        for M in LN_M_SMALL:
            cases.append(_ln_case(M, K, i))
            i += 1
    return cases


def large_case(j, cus):
    """Large case j: row count util_exact_dense.ts_large_m(cus)[j] at K = 128 -- every kloop<G>, a second pass of a block's
    unit loop, a ragged last unit."""
    return _ln_case(X.ts_large_m(cus)[j], 128, j + 1)


def cases(cus):
    return small_cases() + [large_case(j, cus) for j in range(X.TS_LARGE)]


def ln_params(c):
    """(ln_weight, ln_bias) fp16 [256] of a case: fp16(1 + 0.2 randn), fp16(0.1 randn), seeded by the case id."""
    r = X._rng("ln", c["id"])
    return ((1.0 + 0.2 * r.standard_normal(N)).astype(np.float16), (0.1 * r.standard_normal(N)).astype(np.float16))


def pre_norm(c, o):
    """The binary16 pre-norm values of a case, bit for bit (raises util_exact_dense.BudgetError outside the budget)."""
    assert c["N"] == N and not c["relu"] and c["out"] == "fp16"
    pre = X.reference(c, o)
    assert pre.dtype == np.float16
    return pre


def reference(pre, ln_w, ln_b, eps=EPS):
    """LayerNorm over the last axis of the binary16 values `pre` in float64 -> float64 [M, 256]."""
    v = pre.astype(np.float64)
    mean = v.mean(axis=1, keepdims=True)
    d = v - mean
    var = (d * d).mean(axis=1, keepdims=True)
    return d / np.sqrt(var + eps) * ln_w.astype(np.float64) + ln_b.astype(np.float64)


def emulate_f32(pre, ln_w, ln_b, eps=EPS, rstd_ulps=0):
    """The kernel's arithmetic in float32 (sums in float64 rounded once: the summation order is the kernel's business),
    rstd moved by `rstd_ulps` fp32 ulps -> binary16 [M, 256]."""
    f = np.float32
    v = pre.astype(f)
    mean = (v.astype(np.float64).sum(axis=1, keepdims=True) / 256.0).astype(f)
    d = (v - mean).astype(f)
    var = ((d.astype(np.float64) ** 2).sum(axis=1, keepdims=True) / 256.0).astype(f)
    rstd = (1.0 / np.sqrt((var + f(eps)).astype(np.float64))).astype(f)
    step = np.spacing(rstd)
    rstd = (rstd + f(rstd_ulps) * step).astype(f)
    t = (d * rstd).astype(f)
    y = (t.astype(np.float64) * ln_w.astype(np.float64) + ln_b.astype(np.float64)).astype(f)     # one fma
    return y.astype(np.float16)


def ulp16(a):
    """One binary16 ulp at magnitude a (normal range)."""
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def measure(got, want):
    """(largest |got - want| in units of the tolerance, share of outputs that are not the correctly rounded value)."""
    got64 = got.astype(np.float64)
    tol = ulp16(np.maximum(np.abs(want), ULP_FLOOR))
    return float((np.abs(got64 - want) / tol).max()), float((got != want.astype(np.float16)).mean())


def check(got, want, what):
    """The two conditions of the module docstring on binary16 `got` against float64 `want`."""
    assert got.dtype == np.float16 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.isfinite(got.astype(np.float64)).all(), f"{what}: non-finite outputs"
    worst, share = measure(got, want)
    print(f"{what}: worst error {worst:.3f} of the tolerance, {100 * share:.4f} % not correctly rounded")
    if worst > 1.0:
        err = np.abs(got.astype(np.float64) - want) / ulp16(np.maximum(np.abs(want), ULP_FLOOR))
        m, n = np.unravel_index(np.argmax(err), err.shape)
        bad_rows = sorted(set(int(r) for r in np.argwhere(err > 1.0)[:, 0]))
        raise AssertionError(f"{what}: {int((err > 1.0).sum())} outputs beyond one binary16 ulp, worst at [{m}, {n}]: got "
                             f"{got[m, n]!r}, want {want[m, n]!r}; rows {bad_rows[:8]} (units "
                             f"{sorted(set(r // 32 for r in bad_rows))[:8]})")
    if got.shape[0] >= MISROUND_MIN_M:
        assert share <= MISROUND_CAP, f"{what}: {100 * share:.3f} % of the outputs are not the correctly rounded value"
