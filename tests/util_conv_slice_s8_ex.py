"""The cases and statements of bevops_conv_slice_s8_ex's res_first flag (tests/test_conv_slice_s8_ex_gpu.py,
tests/test_deconv_s8_cpu.py): the identity IN FRONT of the activation,

    v = fma(f32(sum), sc, bias);  v = fma(f32(res_q), scale_res, v);  v = act(v);  requantise / round

on the power-of-two lattice of tests/test_conv_slice_s8_gpu.py (scale_a 2^-5, per-channel weight scales, scale_res
2^-5, bias integers * 2^-4: every step is an fp32 number, asserted), next to the order of bevops_conv_slice_s8
(identity BEHIND the activation) on the same operands.  With ReLU the two differ wherever conv + bias is negative and
the identity is not zero -- about half of the outputs; `differing_share` counts them on the statements, so a kernel that
ignores the flag cannot pass."""
import functools

import numpy as np

import util_conv_slice_s8 as S
import util_exact_dense as X

NONE, RELU = 0, 1
S_A, S_RES = 2.0 ** -5, 2.0 ** -5
# (B, H, W, Cin, Cout, ksize): 3 x 3 stride 1 at 64 -> 64 (BasicBlock's conv2) and 1 x 1 at 96 -> 48, on 7 x 9 (63 rows)
# and 12 x 11 (132 rows: across a row-tile edge)
CASES = ((1, 7, 9, 64, 64, 3), (2, 12, 11, 64, 64, 3), (2, 7, 9, 96, 48, 1), (1, 12, 11, 96, 48, 1))


@functools.lru_cache(maxsize=None)
def operands(case):
    B, H, W, Cin, Cout, k = case
    r = X._rng("conv_slice_s8_ex", case)
    x = X.gen_int8(r, (B, H, W, Cin))
    w, ws = X.gen_weights_int8(r, Cout, k * k * Cin, True)
    w = w.reshape(Cout, k, k, Cin)
    bias = X.gen_bias(r, Cout, "s8")
    res = X.gen_identity(r, (B, H, W, Cout), "s8", "int8")
    acc = S.sums(x, w, k, 1)
    for a in (x, w, ws, bias, res, acc):
        a.setflags(write=False)
    return x, w, ws, bias, res, acc


def _finish(v, out, s_out):
    if out == "fp16":
        return v.astype(np.float32).astype(np.float16)
    return np.clip(np.rint(X.f32_exact(v / s_out, "/ scale_out")), -127, 127).astype(np.int8)


def statements(case, act, out):
    """-> (identity in front of the activation, identity behind it, scale_out): int8 or fp16 arrays [B, H, W, Cout]."""
    x, w, ws, bias, res, acc = operands(case)
    v = X.f32_exact(X.f32_exact(acc.astype(np.float64), "(float)sum") * (S_A * ws.astype(np.float64)), "* scale")
    v = X.f32_exact(v + bias.astype(np.float64), "+ bias")
    r = res.astype(np.float64) * S_RES
    front = X.f32_exact(v + r, "+ identity")
    behind = X.f32_exact((np.maximum(v, 0.0) if act == RELU else v) + r, "+ identity behind")
    if act == RELU:
        front = np.maximum(front, 0.0)
    s_out = 2.0 ** int(np.floor(np.log2(front.std() / 48.0))) if out == "int8" else 1.0
    return _finish(front, out, s_out), _finish(behind, out, s_out), s_out


def differing_share(a, b):
    bits = (lambda t: t.view(np.int16)) if a.dtype == np.float16 else (lambda t: t)
    return float((bits(a) != bits(b)).mean())


def order_statement(case, act, out, s_out):
    """The res_first order from the operation-order statement of tests/util_conv_slice_s8.py's fp32 steps."""
    x, w, ws, bias, res, acc = operands(case)
    s_aw, inv = S.host_scalars(S_A, 1.0, s_out if out == "int8" else None)
    sc = (s_aw * S.f32(ws)).astype(np.float32)
    v = S._fma32(acc.astype(np.float32), np.broadcast_to(sc, acc.shape), np.broadcast_to(S.f32(bias), acc.shape))
    v = S._fma32(res.astype(np.float32), np.full(acc.shape, np.float32(S_RES), np.float32), v)
    if act == RELU:
        v = np.maximum(v, np.float32(0))
    if out == "fp16":
        return v.astype(np.float16)
    return np.clip(np.rint((v * inv).astype(np.float32)), -127, 127).astype(np.int8)
