"""Float64 statements, inputs and the interval rule for the two INT8 launches of csrc/lss_split_s8.hip, shared by
tests/test_lss_split_s8_cpu.py (the statements' own properties, the near-tie condition) and tests/test_lss_split_s8_gpu.py.

The interval rule: a byte q agrees with the statement value t (float64, before rounding) when q is the saturating
rounding of SOME point of [t (1 - eps), t (1 + eps)]; eps is derived from the kernel's stated operation order
(design/bevdet_int8.md), never from what the kernel returns."""
import numpy as np

U = 2.0 ** -24          # unit round-off of binary32


def f32_inv(scale):
    """1.f / scale as the host computes it, as a float64 value."""
    return float(np.float32(1.0) / np.float32(scale))


def f32_ratio(scale_b, scale_out):
    """r = scale_b * (1.f / scale_out) in fp32, as a float64 value."""
    return float(np.float32(scale_b) * (np.float32(1.0) / np.float32(scale_out)))


def saturate(t):
    """rne, then the clamp to +-127; NaN -> -127 (the convolution epilogue's rule)."""
    q = np.clip(np.rint(t), -127, 127)
    return np.where(np.isnan(t), -127, q).astype(np.int64)


def interval_ok(q, t, eps):
    """q (integers) against the statement t under the interval rule -> boolean array."""
    a, b = t * (1 - eps), t * (1 + eps)
    lo, hi = saturate(np.minimum(a, b)), saturate(np.maximum(a, b))
    q = np.asarray(q).astype(np.int64)
    return (q >= lo) & (q <= hi)


def near_tie_share(t, eps):
    """Share of the outputs whose interval holds two integers (two roundings are admissible)."""
    a, b = t * (1 - eps), t * (1 + eps)
    return float((saturate(np.minimum(a, b)) != saturate(np.maximum(a, b))).mean())


# ---------------------------------------------------------------------------------------------------- depth split
def softmax64(z):
    """The float64 softmax over the last axis of float64 logits."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(z - z.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)


def depth_statement(logits_f16, scale_depth):
    """t = softmax(x) * (1.f / scale_depth) in float64 for logits [rows, D] (binary16 values)."""
    return softmax64(np.asarray(logits_f16).astype(np.float64)) * f32_inv(scale_depth)


def feat_statement(x_f16, scale_feat):
    return np.asarray(x_f16).astype(np.float64) * f32_inv(scale_feat)


def depth_eps(logits_f16, D):
    """eps of the depth bytes from the operation order: x - m is one rounding of an argument of size <= A (relative
    error A u of the exponential; the maximum's own argument is exactly 0), expf is within 1 ulp = 2 u (the OpenCL /
    HIP device-library bound), both for the numerator and, as a weighted mean, for the denominator; the sum takes
    ceil(D / 4) - 1 additions in a lane and 2 across the quad; one division; one product.  1 % on top for the
    second-order terms."""
    z = np.asarray(logits_f16).astype(np.float64)
    A = float(np.ceil((z.max(axis=-1, keepdims=True) - z).max()))
    assert np.isfinite(A) and A <= 87.0          # e_d stays a normal binary32 number
    return 1.01 * (2 * (2 + A) + (-(-D // 4) + 1) + 2) * U


def gaussian_rows(rows, D, C, stride, doff, foff, seed):
    """Rows [rows, stride] fp16: 3 N(0, 1) logits, N(0, 1) features, every unused column NaN."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.full((rows, stride), float("nan"), dtype=torch.float16)
    x[:, doff:doff + D] = (torch.randn(rows, D, generator=g) * 3).half()
    x[:, foff:foff + C] = torch.randn(rows, C, generator=g).half()
    return x


def exact_rows(rows, D, C, stride, doff, foff, seed):
    """Rows whose bytes are known exactly: k in {1, 2, 4, 8} (k <= D) equal maxima per pixel and every other logit
    -60000 (its exponential underflows to 0 in fp32 and in float64), so every probability is exactly 0 or 1 / k;
    features on the lattice of sixteenths in [-20, 20].  -> (x fp16 [rows, stride], k [rows])."""
    import torch
    rng = np.random.default_rng(seed)
    x = np.full((rows, stride), np.nan, dtype=np.float16)
    ks = [k for k in (1, 2, 4, 8) if k <= D]
    k = np.array([ks[i % len(ks)] for i in range(rows)])
    tops = np.array([-7.25, 0.0, 3.5, 100.0])
    logits = np.full((rows, D), -60000.0)
    for i in range(rows):
        logits[i, rng.choice(D, size=k[i], replace=False)] = tops[i % 4]
    x[:, doff:doff + D] = logits.astype(np.float16)
    x[:, foff:foff + C] = (rng.integers(-320, 321, size=(rows, C)) / 16.0).astype(np.float16)
    # with scale 1 / 8: both saturations, 127 itself, 127.5 (tie, then the clamp), the ties 0.5 -> 0, 1.5 -> 2, -0.5 -> 0
    x[0, foff:foff + 8] = np.array([20.0, -20.0, 15.875, 15.9375, 0.0625, 0.1875, -0.0625, 0.0], dtype=np.float16)
    return torch.from_numpy(x), k


# ------------------------------------------------------------------------------------------------------ up-sampler
def axis_pos(dst, src):
    """Output index -> (i0, i1, weight of i1) of align_corners=True: the exact fraction o (src - 1) / (dst - 1)."""
    o = np.arange(dst, dtype=np.int64)
    if dst == 1:
        z = np.zeros(1, dtype=np.int64)
        return z, z, np.zeros(1)
    num = o * (src - 1)
    i0 = num // (dst - 1)
    lam = (num - i0 * (dst - 1)) / float(dst - 1)
    return i0, np.minimum(i0 + 1, src - 1), lam


def upsample_statement(b, h, w, r):
    """t = bilinear(b) * r in float64 for b int8 [n, hb, wb, C] (numpy) -> [n, h, w, C]."""
    b = np.asarray(b).astype(np.float64)
    y0, y1, ly = axis_pos(h, b.shape[1])
    x0, x1, lx = axis_pos(w, b.shape[2])
    ly, lx = ly.reshape(1, h, 1, 1), lx.reshape(1, 1, w, 1)
    top = (1 - lx) * b[:, y0][:, :, x0] + lx * b[:, y0][:, :, x1]
    bot = (1 - lx) * b[:, y1][:, :, x0] + lx * b[:, y1][:, :, x1]
    return ((1 - ly) * top + ly * bot) * r


def upsample_eps(h, w):
    """eps of the up-sampler's bytes for corners of ONE sign (no cancellation; the model's inputs are behind a ReLU):
    lx = rem / den is one rounding (u); hx = 1 - lx is exact for lx >= 1/2 (Sterbenz) and one rounding otherwise, so
    its relative error is at most u lx / hx + u <= u den (rem <= den - 1); likewise hy.  Each of t, u carries hx's (or
    lx's) error and two roundings, o adds hy's and two more, v one more: (den_x + den_y + 5) u, 1 % on top for the
    second-order terms.  An axis of one output has weight 0 exactly."""
    return 1.01 * ((w - 1) + (h - 1) + 5) * U
