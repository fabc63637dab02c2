"""The statements and operand generators the tests of bevops_deconv4x4s2_s8 share (tests/test_deconv_s8_cpu.py,
tests/test_deconv_s8_gpu.py, tests/test_centernet_int8_gpu.py), from the epilogue operation order of include/bevops.h:

    sc = f32(s_aw * w_scales[co]);  v = fma(f32(sum), sc, bias);  v = max(v, 0) with relu;
    int8: q = clamp(rne(f32(v * inv)), -127, 127), inv = f32(1 / scale_out)          fp16: one rounding of v

* `sums` / `four_gemms_int`: the exact integer sums, as float64 conv_transpose2d and as the kernel's four GEMMs over the
  parity-major packed weight in int64.
* `exact_output`: tests/util_conv_slice_s8.py's (the same fp32 operations, no identity): every output must EQUAL it.
* `linear_interval`: general (non-power-of-two) scales.  The float64 statement v = sum sc + bias, y = act(v),
  t = y / scale_out and the half-width delta of the interval the kernel's fp32 value lies in, DERIVED as
  util_conv_slice_s8.silu_interval derives its own (u = 2^-24):
      e_v   = u (3 P + |v|)(1 + 2^-20)        P = |sum| sc: the two roundings of sc (s_aw on the host, s_aw * w_scales),
                                              the rounding of (float)sum beyond 2^24, and the fma's one rounding of v
      ReLU is 1-Lipschitz: e_y = e_v
      delta = (e_y (1 + 3 u) + 2.01 u |y|) / scale_out     inv's rounding and the product's
  int8 out: the output lies in [clamp(rne(t - delta)), clamp(rne(t + delta))]: at most one step from rne(t), and EQUAL to
  it wherever t is farther than delta from a half-integer.  fp16 out: in [f16(act(v - e_v)), f16(act(v + e_v))]."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import util_conv_slice_s8 as S
import util_exact_dense as X

U = 2.0 ** -24
S_A = 2.0 ** -5
exact_output = S.exact_output


def sums(x_q, w_q):
    """int64 sums [B, 2H, 2W, Cout] of int8 x [B, H, W, Cin] and w [Cin, Cout, 4, 4] (stride 2, padding 1): float64
    conv_transpose2d, exact below 2^53 in any order."""
    y = F.conv_transpose2d(torch.from_numpy(np.asarray(x_q, dtype=np.float64)).permute(0, 3, 1, 2),
                           torch.from_numpy(np.asarray(w_q, dtype=np.float64)), None, stride=2, padding=1)
    y = y.permute(0, 2, 3, 1).numpy()
    assert np.array_equal(y, np.rint(y)) and np.abs(y).max() < 2.0 ** 52
    return y.astype(np.int64)


def four_gemms_int(x_q, packed_q):
    """The kernel's arithmetic in int64: x [B, H, W, Cin] int8, packed [4, Cout, 2, 2, Cin] int8.  Per parity (py, px)
    ONE matrix product of the [B H W, 4 Cin] rows gathered from the zero-padded input (k ordered [dy][dx][Cin], tap
    (dy, dx) = input pixel (y - 1 + py + dy, x - 1 + px + dx)) with the parity's [Cout, 4 Cin] matrix."""
    B, H, W, Cin = x_q.shape
    Cout = packed_q.shape[1]
    xp = np.zeros((B, H + 2, W + 2, Cin), np.int64)
    xp[:, 1:-1, 1:-1] = x_q
    out = np.zeros((B, 2 * H, 2 * W, Cout), np.int64)
    for py in range(2):
        for px in range(2):
            rows = np.concatenate([xp[:, py + dy:py + dy + H, px + dx:px + dx + W] for dy in range(2) for dx in range(2)],
                                  axis=-1).reshape(B * H * W, 4 * Cin)
            prod = rows @ packed_q[2 * py + px].reshape(Cout, 4 * Cin).astype(np.int64).T
            out[:, py::2, px::2] = prod.reshape(B, H, W, Cout)
    return out


def pack(w_q):
    from bevformer_tensorrt_amd.functions.deconv import pack_deconv4x4s2
    return pack_deconv4x4s2(torch.from_numpy(np.array(w_q))).numpy()


# ---------------------------------------------------------------------------------------------- the lattice cases
# (B, H, W, Cin, Cout with int8 out, Cout with fp16 out): a 1 x 1 image at Cin = 64 (one k-step per tap) and Cout = 16;
# 9 x 14 = 126 rows, one short of a tile; 2 x 12 x 11: 132 rows per image, a row-tile edge and an image boundary inside
# a tile, Cout 144 / 136 = a column-tile edge; Cin = 512 (K = 2048).
SHAPES = ((1, 1, 1, 64, 16, 16), (1, 9, 14, 128, 64, 64), (2, 12, 11, 64, 144, 136), (1, 3, 5, 512, 128, 72))
W_AMPS_512 = (64, 31, 7, 1)      # 2048 * 127 * 64 < 2^24: every sum converts to fp32 exactly


def gen_weight(r, Cin, Cout, per_channel):
    """int8 [Cin, Cout, 4, 4] and its scale(s): the amplitude classes of util_exact_dense along dimension 1 (the
    per-channel axis of a transposed convolution's weight) with a power-of-two scale each, or one amplitude and
    scale_w = 2^-9.  -> (w, w_scales or None, scale_w)."""
    amps = W_AMPS_512 if Cin >= 512 else X.W_AMPS
    w = np.empty((Cin, Cout, 4, 4), np.int8)
    for co in range(Cout):
        w[:, co] = X.gen_int8(r, (Cin, 4, 4), amps[co % 4] if per_channel else amps[0])
    if per_channel:
        return w, np.array([X.W_SCALES[co % 4] for co in range(Cout)], np.float32), 1.0
    return w, None, X.S_W


@functools.lru_cache(maxsize=None)
def lattice_case(shape, out, per_channel):
    B, H, W, Cin, c8, c16 = shape
    Cout = c8 if out == "int8" else c16
    r = X._rng("deconv_s8", shape, out, per_channel)
    x = X.gen_int8(r, (B, H, W, Cin))
    w, ws, scale_w = gen_weight(r, Cin, Cout, per_channel)
    bias = X.gen_bias(r, Cout, "s8")
    acc = sums(x, w)
    assert np.abs(acc).max() <= 2 ** 24
    for a in (x, w, bias, acc) + (() if ws is None else (ws,)):
        a.setflags(write=False)
    return x, w, ws, scale_w, bias, acc


def lattice_statement(shape, out, per_channel, with_bias, relu):
    """-> (want, scale_out, t): every step asserted to be an fp32 number, so no contraction can change it."""
    x, w, ws, scale_w, bias, acc = lattice_case(shape, out, per_channel)
    sc = S_A * scale_w * (ws.astype(np.float64) if ws is not None else 1.0)
    v = X.f32_exact(X.f32_exact(acc.astype(np.float64), "(float)sum") * sc, "* scale")
    if with_bias:
        v = X.f32_exact(v + bias.astype(np.float64), "+ bias")
    if relu:
        v = np.maximum(v, 0.0)
    if out == "fp16":
        return v.astype(np.float32).astype(np.float16), 1.0, None
    s_out = 2.0 ** int(np.floor(np.log2(v.std() / 48.0)))
    t = X.f32_exact(v / s_out, "/ scale_out")
    return np.clip(np.rint(t), -127, 127).astype(np.int8), s_out, t


# ---------------------------------------------------------------------------------------------- general scales
GENERAL_CASES = ((2, 12, 11, 64, 144), (1, 9, 14, 128, 64), (1, 3, 5, 512, 144))      # (Cout % 16: int8 out)


@functools.lru_cache(maxsize=None)
def general_case(case):
    B, H, W, Cin, Cout = case
    r = X._rng("deconv_s8 general", case)
    x = np.clip(np.rint(r.normal(0, 40, (B, H, W, Cin))), -127, 127).astype(np.int8)
    w = np.clip(np.rint(r.normal(0, 40, (Cin, Cout, 4, 4))), -127, 127).astype(np.int8)
    scale_a = np.float32(0.0371)
    # pre-activations of a standard deviation around 3
    ws = (r.uniform(0.5, 2.0, Cout) * 3.0 / (40.0 * 40.0 * np.sqrt(4 * Cin) * float(scale_a))).astype(np.float32)
    bias = r.normal(0, 1, Cout).astype(np.float32)
    return x, w, ws, bias, sums(x, w), scale_a


def linear_interval(acc, scale_a, scale_w, w_scales, bias, relu, scale_out):
    """-> (t, delta, lo, hi, y_lo, y_hi): t = y / scale_out float64, delta its half-width in output steps, lo / hi the
    int8 ends; y_lo / y_hi the float64 ends of the value the fp16 output rounds."""
    N = acc.shape[-1]
    sc = float(np.float32(scale_a)) * float(np.float32(scale_w)) * \
        (S.f32(w_scales).astype(np.float64) if w_scales is not None else np.ones(N))
    b = S.f32(bias).astype(np.float64) if bias is not None else np.zeros(N)
    prod = acc.astype(np.float64) * sc
    v = prod + b
    y = np.maximum(v, 0.0) if relu else v
    e_y = U * (3.0 * np.abs(prod) + np.abs(v)) * (1.0 + 2.0 ** -20)
    so = float(np.float32(scale_out))
    t = y / so
    delta = (e_y * (1.0 + 3.0 * U) + 2.01 * U * np.abs(y)) / so
    lo = np.clip(np.rint(t - delta), -127, 127).astype(np.int8)
    hi = np.clip(np.rint(t + delta), -127, 127).astype(np.int8)
    act = (lambda a: np.maximum(a, 0.0)) if relu else (lambda a: a)
    return t, delta, lo, hi, act(v - e_y), act(v + e_y)


def general_statement(case, relu):
    """-> (scale_out, t, delta, lo, hi, y_lo, y_hi) with scale_out = std(y) / 47.3: no power of two, outputs beyond the clamp."""
    x, w, ws, bias, acc, scale_a = general_case(case)
    t0 = linear_interval(acc, scale_a, 1.0, ws, bias, relu, 1.0)[0]
    scale_out = np.float32(t0.std() / 47.3)
    return (scale_out,) + linear_interval(acc, scale_a, 1.0, ws, bias, relu, scale_out)
