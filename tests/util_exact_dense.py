"""Operands on which the int8 / fp16 tiled GEMM family (csrc/tile_gemm.hip, tsgemm_s8_kernel of csrc/tsgemm.hip) makes
NO rounding before its final store, float64 references that predict every output bit, and Python mirrors of the
host-side kernel selection.  Shared by test_dense_exact_cpu.py (which checks all of this without a GPU) and by
test_tile_gemm_exact_gpu.py / test_tsgemm_s8_exact_gpu.py (which compare the kernels with it at tolerance 0).

Why tolerance 0 is legitimate.  The epilogues evaluate, in fp32,

    v = (float)acc * (s_a * s_w[n]) + bias[n] (+ identity[m, n]);  ReLU;  fp16(v)  or  clamp(rint(v * (1 / s_out)))

and the compiler may or may not contract a multiply-add into one FMA.  With every scale a power of two and every
addend on a dyadic grid, each of these intermediates is EXACTLY representable in fp32, so a fused and an unfused
evaluation, and any summation order, give the same bits; the only rounding left is the final one, which the
reference performs once from the exact value.  The reference does not assume this: after each step the kernel performs
in fp32 -- (float)acc, * scale, + bias, + identity, * 1 / s_out -- it checks that the float64 value survives a round trip
through float32 and raises BudgetError otherwise.

Bit budget of the generators below (int8 modes S8 / F16Q):
  * |acc| <= K * 128^2; exact as a float while < 2^24 = 16 777 216, i.e. for every K <= 1 024 whatever the data
    (K * 127^2 = 16 516 096 at K = 1 024).  The dense cases have K <= 512; the 3 x 3 convolutions over 128 channels have
    K = 1 152 (worst case 18.6 M) and stay inside on their random operands (|acc| is a few hundred thousand), which the
    self-check verifies on the actual values.
  * s_a = 2^-5, s_w = 2^-9 per tensor, or per channel 2^-9 / 2^-7 / 2^-5 / 2^-2 for weight amplitudes 127 / 31 / 7 / 1
    (class n % 4: the small-amplitude classes make rounding ties of v / s_out frequent), so acc * scale is acc shifted:
    exact, a multiple of g_n = s_a * s_w[n] >= 2^-14.
  * bias: integers in [-64, 64] times 2^-4; fp16 identity: integers in [-128, 128] times 2^-4; int8 identity times
    s_res = 2^-5; all multiples of every g_n, so every partial result is an integer multiple of g_n of magnitude
    <= |acc| + 2^17 units < 2^24 units: exact.  Largest magnitude: the amplitude-1 class has |acc| <= K * 128 and
    g_n = 2^-7, the others |acc| * g_n <= 2^24 * 2^-10, so |v| <= 16 384 + 20, inside the fp16 range.
  * s_out = 2^-6 .. 2^-3 (by K, so that v / s_out has a standard deviation near 64): v * (1 / s_out) is a shift.
  * F16Q activations (k + t) * s_a, |k| <= 300, t in {0, +-1/4, +-1/2}: 4 (k + t) is an integer below 2^11, so the
    value is an fp16 number; x / s_a = k + t exactly, the half steps are exact rounding ties, |k| > 127 saturates.
fp16 mode (F16): operands are integers in [-8, 8] times 2^-4, products are integers <= 64 in units of 2^-8, and
sum_k |x| |w| <= 864 * 64 units < 2^24: every partial sum is exact in fp32 in any order.  Bias integers in [-256, 256]
times 2^-6, identity integers in [-512, 512] times 2^-5: multiples of 2^-8, total below 2^17 units.

One family is deliberately outside the budget for the accumulator only (saturated_case): K = 2 048, activations all
+127, weights +-127, |acc| up to 33 032 192 > 2^24.  There the reference models (float)acc as the float32
round-to-nearest-even conversion of the exact integer; everything after it is exact again.  Sums formed in fp32 fail.
"""
import zlib

import numpy as np

S8, F16Q, F16 = "S8", "F16Q", "F16"

S_A = 2.0 ** -5
S_W = 2.0 ** -9
S_RES = 2.0 ** -5
W_AMPS = (127, 31, 7, 1)                       # per-channel cases: weight amplitude of channel class n % 4 ...
W_SCALES = (2.0 ** -9, 2.0 ** -7, 2.0 ** -5, 2.0 ** -2)   # ... and its scale (a different power of two per class)


class BudgetError(AssertionError):
    """An intermediate of the reference is not exactly representable in fp32: the operands are outside the budget."""


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _rng(*key):
    return np.random.default_rng(_seed(*key))


def f32_exact(v, what):
    """v (float64) unchanged if every element survives float64 -> float32 -> float64, else BudgetError."""
    v = np.asarray(v, dtype=np.float64)
    back = v.astype(np.float32).astype(np.float64)
    if not np.array_equal(back, v):
        bad = int((back != v).sum())
        raise BudgetError(f"{what}: {bad} of {v.size} values are not fp32 numbers (max |v| {np.abs(v).max():.9g})")
    return v


def s_out_for(K):
    """Power-of-two output scale that leaves values on both sides of the +-127 clamp for a K-deep int8 dot product."""
    return 2.0 ** round(np.log2(np.sqrt(K) * 10.5 * S_A / 64.0))     # v has a standard deviation of about sqrt(K) * 10.5 * s_a


# ---------------------------------------------------------------------------------------------- operand generators
def gen_int8(r, shape, amp=127, plant128=False):
    """int8 uniform in [-amp, amp] with both ends present; plant128: also -128 on ~2 % of the elements."""
    a = r.integers(-amp, amp + 1, size=shape).astype(np.int8)
    flat = a.reshape(-1)
    if flat.size >= 2:
        flat[-1], flat[flat.size // 2] = amp, -amp
    if plant128:
        flat[r.random(flat.size) < 0.02] = -128
        flat[0] = -128
    return a


def gen_weights_int8(r, N, K, per_channel, plant128=False):
    """[N, K] int8 weights and their scale(s): full range with one scale, or amplitude classes with a scale each."""
    if not per_channel:
        return gen_int8(r, (N, K), 127, plant128), S_W
    w = np.empty((N, K), dtype=np.int8)
    for n in range(N):
        w[n] = gen_int8(r, (K,), W_AMPS[n % 4], plant128 and n % 4 == 0)
    return w, np.array([W_SCALES[n % 4] for n in range(N)], dtype=np.float32)


def gen_f16q_acts(r, shape, s_a=S_A):
    """fp16 activations on the tie grid (k + t) * s_a: t = +-1/2 are exact rounding ties, |k| up to 300 saturates."""
    wide = r.random(shape) < 0.15
    k = np.where(wide, r.integers(-300, 301, size=shape), r.integers(-130, 131, size=shape))
    t = r.choice(np.array([0.0, 0.25, -0.25, 0.5, -0.5]), size=shape)
    x = (k + t) * s_a
    flat = x.reshape(-1)
    if flat.size >= 4:
        flat[-1], flat[-2], flat[0], flat[1] = 300.5 * s_a, -300.5 * s_a, 2.5 * s_a, -3.5 * s_a
    x16 = x.astype(np.float16)
    if not np.array_equal(x16.astype(np.float64), x):
        raise BudgetError("tie grid is not representable in fp16")
    return x16


def gen_f16_small(r, shape):
    """fp16 operands of the F16 mode: integers in [-8, 8] times 2^-4."""
    return (r.integers(-8, 9, size=shape) * 2.0 ** -4).astype(np.float16)


def gen_bias(r, N, mode):
    if mode == F16:
        return (r.integers(-256, 257, size=N) * 2.0 ** -6).astype(np.float16)
    return (r.integers(-64, 65, size=N) * 2.0 ** -4).astype(np.float32)


def gen_identity(r, shape, mode, kind):
    """kind 'fp16': dyadic fp16 rows; 'int8': int8 rows (real value q * S_RES)."""
    if kind == "int8":
        return gen_int8(r, shape)
    if mode == F16:
        return (r.integers(-512, 513, size=shape) * 2.0 ** -5).astype(np.float16)
    return (r.integers(-128, 129, size=shape) * 2.0 ** -4).astype(np.float16)


# ---------------------------------------------------------------------------------------------------- references
def ref_quantize(x, s_a):
    """The F16Q quantiser and bevops_quantize_rows: clamp(rint(x / s_a), -127, 127), ties to even."""
    return np.clip(np.rint(np.asarray(x, dtype=np.float64) / s_a), -127, 127).astype(np.int8)


def ref_dequantize(q, s):
    """bevops_dequantize_rows: fp16(q * s), the product exact in fp32 for a power-of-two s, one rounding."""
    return f32_exact(np.asarray(q, dtype=np.float64) * s, "q * scale").astype(np.float32).astype(np.float16)


def ref_epilogue(acc, scale, bias, res, relu, out, s_out=1.0, acc_rne=False):
    """acc float64 [M, N] (exact sums) -> the kernel's output bits.  scale: s_a * s_w (float or [N]); bias [N] or
    None; res: real values of the identity rows [M, N] (float64) or None; out 'fp16' | 'int8'.
    acc_rne: model (float)acc as the float32 RNE conversion instead of requiring it to be exact."""
    acc = np.asarray(acc, dtype=np.float64)
    v = acc.astype(np.float32).astype(np.float64) if acc_rne else f32_exact(acc, "(float)acc")
    v = f32_exact(v * np.asarray(scale, dtype=np.float64), "* scale")
    if bias is not None:
        v = f32_exact(v + np.asarray(bias, dtype=np.float64), "+ bias")
    if res is not None:
        v = f32_exact(v + res, "+ identity")
    if relu:
        v = np.maximum(v, 0.0)
    if out == "fp16":
        return v.astype(np.float32).astype(np.float16)          # the ONE rounding (float64 -> float32 is exact here)
    t = f32_exact(v * (1.0 / s_out), "* 1 / s_out")
    return np.clip(np.rint(t), -127, 127).astype(np.int8)


def exact_value(acc, scale, bias, res, relu):
    """The exact pre-rounding value of ref_epilogue (for the tie / inexact statistics)."""
    v = np.asarray(acc, dtype=np.float64) * np.asarray(scale, dtype=np.float64)
    if bias is not None:
        v = v + np.asarray(bias, dtype=np.float64)
    if res is not None:
        v = v + res
    return np.maximum(v, 0.0) if relu else v


def fp16_shares(v):
    """(share of exact values that are not fp16 numbers, share that are exact fp16 ties) of float64 v."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    h = v.astype(np.float16).astype(np.float64)
    inexact = h != v
    up = np.nextafter(h.astype(np.float16), np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(h.astype(np.float16), np.float16(-np.inf)).astype(np.float64)
    other = np.where(v > h, up, dn)
    tie = inexact & (np.abs(v - h) == np.abs(other - v))
    return float(inexact.mean()), float(tie.mean())


def int8_shares(t):
    """(share of v / s_out that are rounding ties, share beyond +-127) of float64 t = v / s_out."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    return float((np.abs(t - np.floor(t) - 0.5) == 0).mean()), float((np.abs(t) > 127).mean())


def int_matmul(a, w):
    """sum_k a[m, k] w[n, k] in float64: exact below 2^53 in any order."""
    return np.asarray(a, dtype=np.float64) @ np.asarray(w, dtype=np.float64).T


def int_conv(x_nhwc, w_taps, ks, stride):
    """Convolution (pad ks // 2) of x [B, H, W, Cin] with w [Cout, ks, ks, Cin] in float64 -> [B * Ho * Wo, Cout]."""
    import torch
    x = torch.from_numpy(np.asarray(x_nhwc, dtype=np.float64)).permute(0, 3, 1, 2)
    w = torch.from_numpy(np.asarray(w_taps, dtype=np.float64)).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(x, w, None, stride, ks // 2)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0]).numpy()


def conv_out_hw(H, W, ks, stride):
    pad = ks // 2
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


# ------------------------------------------------------------------------------------------------ cases
def _case(**kw):
    c = dict(mode=S8, conv=False, M=0, N=0, K=0, bias=False, per_channel=False, relu=False, res=None, out="fp16",
             plant128=False, sat=False)
    c.update(kw)
    if c["conv"]:
        ho, wo = conv_out_hw(c["H"], c["W"], c["ks"], c["stride"])
        c["M"], c["N"], c["K"] = c["B"] * ho * wo, c["Cout"], c["ks"] * c["ks"] * c["Cin"]
        c["id"] = (f"{c['mode']}-conv{c['ks']}s{c['stride']}-{c['B']}x{c['H']}x{c['W']}x{c['Cin']}-{c['Cout']}"
                   f"-{_flags(c)}")
    else:
        c["id"] = f"{c['mode']}-{c['M']}x{c['N']}x{c['K']}-{_flags(c)}"
    return c


def _flags(c):
    return "".join([("b" if c["bias"] else ""), ("c" if c["per_channel"] else ""), ("r" if c["relu"] else ""),
                    {None: "", "fp16": "I", "int8": "Q"}[c["res"]], ("8" if c["out"] == "int8" else "h"),
                    ("m" if c["plant128"] else ""), ("S" if c["sat"] else "")])


GEMM_M = (1, 63, 65, 127, 128, 129, 257)
GEMM_N = (1, 9, 100, 64, 72, 128, 136)
GEMM_K8 = (16, 48, 64, 80, 128, 144, 192)
GEMM_K16 = (8, 24, 32, 40, 96)
TILE_ORDER_SHAPE = (385, 384, 64)      # 4 x 3 = 12 tiles: per_xcd = 2, grid 16, four blocks return early


def gemm_cases():
    """Dense cases of test_tile_gemm_exact_gpu.py: every (N, K) pair of the edge lists per mode, M and the epilogue flags
    cycling with co-prime periods (test_dense_exact_cpu.py checks that every flag value meets a ragged M, a ragged N and
    a K tail, and that all non-convolution instantiations are reached)."""
    cases = []
    for mode, ks in ((S8, GEMM_K8), (F16Q, GEMM_K8), (F16, GEMM_K16)):
        i = 0
        for jn, N in enumerate(GEMM_N):
            for jk, K in enumerate(ks):
                M = GEMM_M[(2 * jn + 3 * jk + (1 if mode == F16Q else 0)) % 7]
                res = (None, "fp16", "int8")[i % 3]
                if res == "int8" and mode != S8:
                    res = "fp16" if i % 2 else None
                cases.append(_case(mode=mode, M=M, N=N, K=K, bias=i % 2 == 0, per_channel=mode != F16 and i % 4 < 2,
                                   relu=i % 5 < 2, res=res, out="int8" if mode != F16 and (i // 3) % 2 else "fp16",
                                   plant128=mode == S8 and i % 8 == 5))
                i += 1
        M, N, K = TILE_ORDER_SHAPE
        cases.append(_case(mode=mode, M=M, N=N, K=K if mode != F16 else 32, bias=True, per_channel=mode != F16,
                           res="fp16"))
    return cases


CONV_IMAGES = ((1, 1), (1, 6), (5, 1), (5, 3), (7, 9))       # B = 3; 7 x 9: Hout * Wout = 63, a row tile spans images
CONV_COUT = (8, 20, 64, 136)


def conv_cases():
    """Implicit-convolution cases: every (image, kernel size, stride) per mode, channels and flags cycling."""
    cases = []
    for mode, cins in ((S8, (64, 128)), (F16Q, (64, 128)), (F16, (32, 96))):
        i = 0
        for (H, W) in CONV_IMAGES:
            for ks in (1, 3):
                for stride in (1, 2, 3):
                    out = "int8" if mode == S8 and i % 2 == 0 else "fp16"
                    cases.append(_case(mode=mode, conv=True, B=3, H=H, W=W, Cin=cins[(i // 2) % 2],
                                       Cout=CONV_COUT[(i + i // 4) % 4], ks=ks, stride=stride, bias=i % 3 != 2,
                                       per_channel=mode != F16 and i % 4 < 2, relu=out == "int8" or i % 5 == 1,
                                       res="fp16" if i % 3 == 1 else None, out=out))
                    i += 1
    return cases


def saturated_cases():
    """K = 2 048, activations all +127, weights +-127: |acc| up to 33 032 192 > 2^24, no bias, no identity.  Channel
    class n % 4: all +127 / all -127 / +127 with 3 % of the signs flipped / all of one sign with one weight of +-126, which
    makes acc ODD and therefore an exact tie of the int32 -> float32 conversion.  N = 72: the tiled kernel; N = 256: also tsgemm_s8."""
    return [_case(mode=S8, M=40, N=N, K=2048, out=out, sat=True) for N in (72, 256) for out in ("fp16", "int8")]


TS_N = (256, 512)
TS_K = (128, 256, 384, 512)
TS_M_SMALL = (1, 31, 33, 160)


def ts_large_m(cus):
    """Row counts for tsgemm_s8 computed from the CU count, each with a ragged last unit (M % 32 == 17):
    1.5, 3.5 and 5.5 units per block -> G in {1, 2}, {3, 4} and {5, then a second pass of 1}; 7 units per block -> a
    second pass of 2."""
    half = cus // 2
    return [32 * (cus + half) - 15, 32 * (3 * cus + half) - 15, 32 * (5 * cus + half) - 15, 32 * 7 * cus - 15]


def ts_expected_partition(cus):
    """What ts_s8_partition must report for ts_large_m(cus): per M the set of per-block pass tuples."""
    return [{(1,), (2,)}, {(3,), (4,)}, {(5,), (5, 1)}, {(5, 2)}]


def ts_small_cases():
    """Every (M, N, K) of the small lists with the flags cycling: one unit count per block (G = 1), whatever the device."""
    cases, i = [], 0
    for N in TS_N:
        for K in TS_K:
            for M in TS_M_SMALL:
                cases.append(_case(mode=S8, M=M, N=N, K=K, bias=i % 2 == 0, per_channel=i % 4 < 2, relu=i % 5 < 2,
                                   res=(None, "fp16", "int8")[i % 3], out="int8" if (i // 3) % 2 else "fp16",
                                   plant128=i % 8 == 5))
                i += 1
    return cases


TS_LARGE = 4      # len(ts_large_m(cus))


def ts_large_case(j, cus):
    """Large case j: row count ts_large_m(cus)[j] at K = 128, N = 256."""
    return _case(mode=S8, M=ts_large_m(cus)[j], N=256, K=128, bias=True, per_channel=j % 2 == 0, relu=j % 2 == 1,
                 res=("int8", "fp16", None, "int8")[j], out=("int8", "fp16", "int8", "fp16")[j])


def ts_cases(cus):
    """All cases of test_tsgemm_s8_exact_gpu.py on a device with `cus` compute units."""
    return ts_small_cases() + [ts_large_case(j, cus) for j in range(TS_LARGE)]


# ------------------------------------------------------------------------------- operands and reference of a case
def make_ops(c):
    """All operands of a case as numpy arrays (seeded by the case id): a (int8 [M, K] / fp16; convolution: [B, H, W, Cin]),
    w ([N, K]; convolution: [Cout, ks, ks, Cin]), s_a, s_w (float or fp32 [N]), bias, res, s_res, s_out."""
    r = _rng(c["id"])
    mode, N, K = c["mode"], c["N"], c["K"]
    ashape = (c["B"], c["H"], c["W"], c["Cin"]) if c["conv"] else (c["M"], K)
    o = dict(s_a=S_A, s_w=S_W, s_res=S_RES, s_out=s_out_for(K), bias=None, res=None)
    if c["sat"]:
        o["a"] = np.full(ashape, 127, dtype=np.int8)
        n = np.arange(N)
        w = np.where(r.random((N, K)) < 0.03, -127, 127)            # class 2: a few signs flipped, acc stays > 2^24
        w[n % 4 == 0], w[n % 4 == 1] = 127, -127
        w[n % 8 == 3], w[n % 8 == 7] = 127, -127
        w[n % 8 == 3, 5], w[n % 8 == 7, 5] = 126, -126              # class 3: acc odd
        o["w"], o["s_w"], o["s_out"] = w.astype(np.int8), 2.0 ** -6, 2.0 ** 7
        return o
    if mode == F16:
        o["a"], o["w"] = gen_f16_small(r, ashape), gen_f16_small(r, (N, K))
        o["s_a"] = o["s_w"] = 1.0
    else:
        o["a"] = gen_f16q_acts(r, ashape) if mode == F16Q else gen_int8(r, ashape, 127, c["plant128"])
        o["w"], o["s_w"] = gen_weights_int8(r, N, K, c["per_channel"], c["plant128"])
    if c["conv"]:
        o["w"] = np.ascontiguousarray(o["w"].reshape(N, c["ks"], c["ks"], c["Cin"]))
    if c["bias"]:
        o["bias"] = gen_bias(r, N, mode)
    if c["res"]:
        o["res"] = gen_identity(r, (c["M"], N), mode, c["res"])
    return o


def case_acc(c, o):
    """The exact sums of a case, float64 [M, N] (F16Q: over the reference quantiser's integers)."""
    a = ref_quantize(o["a"], o["s_a"]) if c["mode"] == F16Q else o["a"]
    if c["mode"] == F16:
        aa, ww = np.abs(a.astype(np.float64)), np.abs(o["w"].astype(np.float64))
        worst = (int_conv(aa, ww, c["ks"], c["stride"]) if c["conv"] else int_matmul(aa, ww)).max()
        if worst * 2.0 ** 8 >= 2.0 ** 24:
            raise BudgetError(f"fp16 mode: sum |x||w| = {worst} is not below 2^16")
    return int_conv(a, o["w"], c["ks"], c["stride"]) if c["conv"] else int_matmul(a, o["w"])


def case_terms(c, o):
    """(acc, scale, bias, res) of a case as the float64 terms of ref_epilogue."""
    scale = 1.0 if c["mode"] == F16 else np.float64(o["s_a"]) * np.asarray(o["s_w"], dtype=np.float64)
    res = None
    if o["res"] is not None:
        res = o["res"].astype(np.float64) * (o["s_res"] if c["res"] == "int8" else 1.0)
    return case_acc(c, o), scale, o["bias"], res


def reference(c, o):
    """The output bits of a case: fp16 or int8 [M, N]."""
    acc, scale, bias, res = case_terms(c, o)
    return ref_epilogue(acc, scale, bias, res, c["relu"], c["out"], o["s_out"], acc_rne=c["sat"])


# ------------------------------------------------------------------------- mirrors of the host-side selection
def tile_instance(mode, conv, out8, res8, N):
    """The tile_gemm_kernel<MODE, OUT8, NI, CONV, RES8> instantiation launch_tile_gemm picks (csrc/tile_gemm.hip, the
    BEVOPS_TG dispatch), or None where the launch code returns a status instead."""
    ni = 1 if N <= 64 else 2                    # `narrow`: 64-column tiles
    conv, out8, res8 = bool(conv), bool(out8), bool(res8)
    if res8 and (mode != S8 or conv):
        return None
    if mode == F16:
        return None if out8 else (F16, False, ni, conv, False)
    if mode == F16Q:
        if conv:
            return None if out8 else (F16Q, False, ni, True, False)
        return (F16Q, out8, ni, False, False)
    if conv:
        return (S8, out8, ni, True, False)
    return (S8, out8, ni, False, res8)


ALL_TILE_INSTANCES = frozenset(
    (mode, out8, ni, conv, res8)
    for ni in (1, 2)
    for (mode, out8, conv, res8) in (
        (F16, False, True, False), (F16, False, False, False),
        (F16Q, False, True, False), (F16Q, True, False, False), (F16Q, False, False, False),
        (S8, True, True, False), (S8, False, True, False), (S8, True, False, True), (S8, True, False, False),
        (S8, False, False, True), (S8, False, False, False)))


def case_instance(c):
    return tile_instance(c["mode"], c["conv"], c["out"] == "int8", c["res"] == "int8", c["N"])


TS_G = 5      # kTsG: row units a block multiplies at a time


def ts_s8_partition(M, cus):
    """tsgemm_s8_kernel's split of ceil(M / 32) row units over min(units, cus) blocks, with the kernel's
    per / extra / u_begin / u_end arithmetic: the list of (block, G) passes in launch order."""
    units = (M + 31) // 32
    nb = min(units, cus)
    per, extra = units // nb, units % nb
    passes = []
    for bi in range(nb):
        u_begin = bi * per + min(bi, extra)
        u_end = u_begin + per + (1 if bi < extra else 0)
        for u0 in range(u_begin, u_end, TS_G):
            passes.append((bi, min(TS_G, u_end - u0)))
    return passes


def ts_block_passes(M, cus):
    """The set of per-block G tuples of ts_s8_partition(M, cus), e.g. {(5,), (5, 1)}."""
    per_block = {}
    for bi, g in ts_s8_partition(M, cus):
        per_block.setdefault(bi, []).append(g)
    return {tuple(v) for v in per_block.values()}
