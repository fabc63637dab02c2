"""The statements the tests of bevops_conv_slice_s8 compare with (tests/test_conv_slice_s8_gpu.py,
tests/test_yolox_int8_gpu.py), from the epilogue operation order documented in include/bevops.h:

    sc = f32(s_aw * w_scales[co]);  v = fma(f32(sum), sc, bias);  v = act(v);  v = fma(f32(res_q), scale_res, v);
    int8: q = clamp(rne(f32(v * inv)), -127, 127), inv = f32(1 / scale_out)          fp16: one rounding of v

* `exact_output` (act none / ReLU): the fp32 operations themselves, each evaluated in the extended type (64-bit
  significand) and rounded once to fp32 -- a product of two fp32 numbers (48 bits) is exact there; a fused multiply-add
  differs from the fp32 result only when the extended sum lies within 2^-64 relative of an fp32 rounding tie without
  being one.  Every output must EQUAL it.
* `silu_interval`: the float64 statement t = (silu(v) + res) / scale_out and the half-width delta of the interval the
  kernel's fp32 value lies in, DERIVED (design/yolox_int8.md section 5), in output steps:
      e_v = u (3 P + |v|)(1 + 2^-20)          P = |sum| sc: two roundings of sc, (float)sum, the fma's one rounding
      e_a = 1.1 e_v + 2^-17 (|silu(v)| + 1.1 e_v) + 2^-120       |silu'| <= 1.1; the SiLU evaluation bound of
                                                                  design/yolox.md (2^-17 relative)
      e_y = e_a + u (|silu(v) + r| + e_a)                         the identity's fma: one rounding
      delta = (e_y (1 + 3 u) + 2.01 u |y|) / scale_out            inv's rounding and the product's
  with u = 2^-24.  The output must lie in [clamp(rne(t - delta)), clamp(rne(t + delta))]; where the two ends differ the
  value is within delta of a half-integer and one step either way is allowed."""
import numpy as np

import util_exact_dense as X

U = 2.0 ** -24
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the exact statement needs the 64-bit significand of the x87 extended type"


def f32(v):
    return np.asarray(v).astype(np.float32)


def sums(x_q, w_q, k, stride):
    """int64 sums [B, Ho, Wo, Cout] of int8 x [B, H, W, Cin] and w [Cout, k, k, Cin] (exact: float64 below 2^53)."""
    B, H, W, _ = x_q.shape
    Ho, Wo = X.conv_out_hw(H, W, k, stride)
    s = X.int_conv(x_q, w_q, k, stride).reshape(B, Ho, Wo, w_q.shape[0])
    assert np.array_equal(s, np.rint(s))
    return s.astype(np.int64)


def host_scalars(scale_a, scale_w, scale_out):
    """(s_aw, inv) as the entry computes them on the host in fp32."""
    s_aw = np.float32(scale_a) * np.float32(scale_w)
    inv = np.float32(1.0) / np.float32(scale_out) if scale_out is not None else np.float32(1.0)
    return np.float32(s_aw), np.float32(inv)


def _fma32(a, b, c):
    """f32(a * b + c) for fp32 arrays: product exact in the extended type, one rounding there, one to fp32."""
    return (a.astype(LD) * b.astype(LD) + c.astype(LD)).astype(np.float32)


def exact_output(acc, scale_a, scale_w, w_scales, bias, act, res_q, scale_res, scale_out, out):
    """acc int64 [..., Cout]; act 0 / 1; out 'int8' | 'fp16' -> the kernel's output (int8 or fp16 array)."""
    assert act in (0, 1)
    s_aw, inv = host_scalars(scale_a, scale_w, scale_out if out == "int8" else None)
    N = acc.shape[-1]
    sc = (s_aw * f32(w_scales)).astype(np.float32) if w_scales is not None else np.full(N, s_aw, np.float32)
    b = f32(bias) if bias is not None else np.zeros(N, np.float32)
    v = _fma32(acc.astype(np.float32), np.broadcast_to(sc, acc.shape), np.broadcast_to(b, acc.shape))
    if act == 1:
        v = np.maximum(v, np.float32(0))
    if res_q is not None:
        v = _fma32(res_q.astype(np.float32), np.full(acc.shape, np.float32(scale_res), np.float32), v)
    if out == "fp16":
        return v.astype(np.float16)
    t = (v * inv).astype(np.float32)
    return np.clip(np.rint(t), -127, 127).astype(np.int8)


def silu64(v):
    return v / (1.0 + np.exp(-v))


def silu_interval(acc, scale_a, scale_w, w_scales, bias, res_q, scale_res, scale_out):
    """-> (t float64, delta float64, lo int8, hi int8) of the SiLU epilogue with int8 output."""
    N = acc.shape[-1]
    sc = float(np.float32(scale_a)) * float(np.float32(scale_w)) * \
        (f32(w_scales).astype(np.float64) if w_scales is not None else np.ones(N))
    b = f32(bias).astype(np.float64) if bias is not None else np.zeros(N)
    prod = acc.astype(np.float64) * sc
    v = prod + b
    a = silu64(v)
    r = res_q.astype(np.float64) * float(np.float32(scale_res)) if res_q is not None else 0.0
    y = a + r
    so = float(np.float32(scale_out))
    t = y / so
    e_v = U * (3.0 * np.abs(prod) + np.abs(v)) * (1.0 + 2.0 ** -20)
    e_a = 1.1 * e_v + 2.0 ** -17 * (np.abs(a) + 1.1 * e_v) + 2.0 ** -120
    e_y = e_a + (U * (np.abs(y) + e_a) if res_q is not None else 0.0)
    delta = (e_y * (1.0 + 3.0 * U) + 2.01 * U * np.abs(y)) / so
    lo = np.clip(np.rint(t - delta), -127, 127).astype(np.int8)
    hi = np.clip(np.rint(t + delta), -127, 127).astype(np.int8)
    return t, delta, lo, hi


def check_interval(got, lo, hi, cap=0.01):
    """got inside [lo, hi] everywhere; the share of excused outputs (lo != hi) at most `cap`.  -> that share."""
    bad = np.argwhere((got < lo) | (got > hi))
    assert len(bad) == 0, (f"{len(bad)} of {got.size} outputs outside their interval, first at {tuple(bad[0])}: got "
                           f"{got[tuple(bad[0])]}, allowed {lo[tuple(bad[0])]} .. {hi[tuple(bad[0])]}")
    share = float((lo != hi).mean())
    assert share <= cap, f"{share:.4%} of the outputs lie within delta of a half-integer (cap {cap:.0%})"
    return share
