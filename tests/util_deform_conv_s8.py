"""The statements the tests of bevops_deform_conv3x3_nhwc_s8 compare with (tests/test_deform_conv_s8_cpu.py,
tests/test_deform_conv_s8_gpu.py, tests/test_bevdepth_dcn_int8_gpu.py), from the operation order of include/bevops.h:

    positions, fractions and the four corner weights in numpy float32 with the kernel's operations (exact reproduction);
    s = w00 v00 + w01 v01 + w10 v10 + w11 v11 in float64 from them: EXACT (a 24-bit x 8-bit product fits, and so do the
        sums), where the kernel takes four fp32 operations;
    c = clamp(rne(s), -127, 127);  sum = the int64 sum over (tap, channel of the group);  then bevops_conv_slice_s8's
        epilogue (tests/util_conv_slice_s8.py: `exact_output`).

ON THE LATTICE (offsets multiples of 1 / 64 in [-4, 4)) positions, fractions (6 bits) and corner weights (<= 13 bits)
are exact; every product with an int8 value and every partial sum is a multiple of 2^-12 of magnitude <= 128, <= 20
significant bits, so the kernel's fp32 blend is exact and rne(s) is the exact rational's rounding, true ties included:
every column byte EQUALS the statement.  With GENERAL fp16 offsets the kernel's s differs from the float64 one by at
most four fp32 roundings of magnitudes <= 127: EPS = 4 * 2^-24 * 127; a byte must equal rne(s64) except where s64 lies
within EPS of a half-integer, where either neighbour passes (`column_interval`)."""
import functools

import numpy as np

import util_conv_slice_s8 as S
import util_exact_dense as X

TAPS = 9
EPS = 4 * 2.0 ** -24 * 127
NEAR_TIE_CAP = 1e-3                      # share of a general-offset case within EPS of a half-integer (expected ~6e-5)
U = 2.0 ** -24

# (Cin / groups, Cout / groups, groups): 96 covers the 32-byte k-chunk and the half-empty second channel tile
CHANNELS = ((32, 32, 1), (64, 64, 4), (96, 32, 2), (32, 96, 2), (64, 96, 1), (96, 96, 4))
# (B, H, W): one pixel, every tap partly outside; 270 pixels: tiles cross the image boundary, the tail has 14 rows
PIXELS = ((1, 1, 1), (2, 9, 15))
S_A = 2.0 ** -5


def positions(off16, H, W):
    """off16 [B, H, W, >= 18] float16 -> (idx [B, H, W, 9, 4] int64: the corner's pixel inside its image, 0 where the
    corner is not read; wgt [B, H, W, 9, 4] float32: its weight, 0 where it is not read; live [B, H, W, 9])."""
    off = np.asarray(off16)[..., :2 * TAPS].astype(np.float32)
    i, j = np.divmod(np.arange(TAPS), 3)
    y = np.arange(H)[None, :, None, None]
    x = np.arange(W)[None, None, :, None]
    one, zero = np.float32(1), np.float32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        h = (y - 1 + i).astype(np.float32) + off[..., 0::2]
        w = (x - 1 + j).astype(np.float32) + off[..., 1::2]
        live = (h > -1) & (w > -1) & (h < H) & (w < W)
    h, w = np.where(live, h, zero), np.where(live, w, zero)
    hf, wf = np.floor(h), np.floor(w)
    lh, lw = h - hf, w - wf
    hh, hw = one - lh, one - lw
    assert lh.dtype == np.float32 and hh.dtype == np.float32
    wgt = np.stack([hh * hw, hh * lw, lh * hw, lh * lw], axis=-1)
    h0, w0 = hf.astype(np.int64), wf.astype(np.int64)
    hs = np.stack([h0, h0, h0 + 1, h0 + 1], axis=-1)
    ws = np.stack([w0, w0 + 1, w0, w0 + 1], axis=-1)
    ok = live[..., None] & (hs >= 0) & (hs <= H - 1) & (ws >= 0) & (ws <= W - 1)
    return np.where(ok, hs * W + ws, 0), np.where(ok, wgt, zero).astype(np.float32), live


def column_s64(x_q, off16):
    """x_q int8 [B, H, W, C], off16 [B, H, W, >= 18] -> s float64 [B, H, W, 9, C]: the exact blend."""
    B, H, W, C = x_q.shape
    idx, wgt, _ = positions(off16, H, W)
    flat = np.asarray(x_q).reshape(B, H * W, C).astype(np.float64)
    s = np.zeros((B, H, W, TAPS, C))
    for q in range(4):
        v = np.stack([flat[b][idx[b, ..., q]] for b in range(B)])            # [B, H, W, 9, C]
        s += wgt[..., q, None].astype(np.float64) * v
    return s


def column(s64):
    """The column bytes of the exact blend: clamp(rne(s), -127, 127)."""
    return np.clip(np.rint(s64), -127, 127).astype(np.int8)


def near_tie(s64, eps=EPS):
    """Where s64 lies within eps of a half-integer WITHOUT being decided: either neighbour passes there."""
    return np.abs(s64 - np.floor(s64) - 0.5) <= eps


def column_interval(s64, eps=EPS):
    """-> (lo, hi) int8: the bytes a kernel may leave for the exact blend s64."""
    lo = np.clip(np.rint(s64 - eps), -127, 127).astype(np.int8)
    hi = np.clip(np.rint(s64 + eps), -127, 127).astype(np.int8)
    return lo, hi


def sums(col, w_q, groups):
    """int64 [B, H, W, Cout] of the column bytes [B, H, W, 9, Cin] and w_q int8 [Cout, 3, 3, Cin / groups]."""
    B, H, W, _, Cin = col.shape
    Cout, cin_g = w_q.shape[0], w_q.shape[3]
    assert cin_g * groups == Cin and Cout % groups == 0
    cout_g = Cout // groups
    wk = np.asarray(w_q).reshape(Cout, TAPS, cin_g).astype(np.float64)
    out = np.empty((B, H, W, Cout))
    for g in range(groups):
        c = col[..., g * cin_g:(g + 1) * cin_g].astype(np.float64).reshape(B * H * W, TAPS * cin_g)
        out[..., g * cout_g:(g + 1) * cout_g] = (c @ wk[g * cout_g:(g + 1) * cout_g].reshape(cout_g, -1).T).reshape(B, H, W, cout_g)
    assert np.abs(out).max(initial=0) < 2.0 ** 31
    return out.astype(np.int64)


def statement(x_q, off16, w_q, groups, scale_a, w_scales, bias, relu, scale_out, out, scale_w=1.0):
    """The whole entry on the exact blend -> (output int8 / fp16 [B, H, W, Cout], s64, sums)."""
    s64 = column_s64(x_q, off16)
    acc = sums(column(s64), w_q, groups)
    return S.exact_output(acc, scale_a, scale_w, w_scales, bias, int(relu), None, 1.0, scale_out, out), s64, acc


def linear_interval(acc, scale_a, scale_w, w_scales, bias, relu, scale_out):
    """util_conv_slice_s8.silu_interval without the SiLU and the identity: t = act(sum sc + bias) / scale_out in float64
    and the half-width of the interval the kernel's fp32 value lies in, in output steps:
        e_v = u (3 P + |v|)(1 + 2^-20)          P = |sum| sc: two roundings of sc, (float)sum, the fma's one rounding
        delta = (e_v (1 + 3 u) + 2.01 u |v|) / scale_out            inv's rounding and the product's
    -> (t, delta, lo int8, hi int8)."""
    N = acc.shape[-1]
    sc = float(np.float32(scale_a)) * float(np.float32(scale_w)) * \
        (S.f32(w_scales).astype(np.float64) if w_scales is not None else np.ones(N))
    b = S.f32(bias).astype(np.float64) if bias is not None else np.zeros(N)
    prod = acc.astype(np.float64) * sc
    v = prod + b
    e_v = U * (3.0 * np.abs(prod) + np.abs(v)) * (1.0 + 2.0 ** -20)
    if relu:
        v = np.maximum(v, 0.0)
    so = float(np.float32(scale_out))
    t = v / so
    delta = (e_v * (1.0 + 3.0 * U) + 2.01 * U * np.abs(v)) / so
    lo = np.clip(np.rint(t - delta), -127, 127).astype(np.int8)
    hi = np.clip(np.rint(t + delta), -127, 127).astype(np.int8)
    return t, delta, lo, hi


# ---------------------------------------------------------------------------------------------- operands
def lattice_offsets(r, B, H, W, channels=18):
    """Multiples of 1 / 64 in [-4, 4) as fp16 (exact), [B, H, W, channels]; a quarter of them on halves and whole
    numbers, so that true rounding ties of the blend and integer positions occur."""
    k = r.integers(-256, 256, size=(B, H, W, channels))
    coarse = r.random(k.shape) < 0.25
    k = np.where(coarse, k // 32 * 32, k)
    o = (k / 64.0).astype(np.float16)
    assert np.array_equal(o.astype(np.float64) * 64, k)
    return o


def general_offsets(r, B, H, W, channels=18):
    """Gaussian fp16 offsets, sigma one pixel."""
    return r.normal(0.0, 1.0, size=(B, H, W, channels)).astype(np.float16)


@functools.lru_cache(maxsize=None)
def lattice_case(ch, px):
    """(x int8, off fp16 [.., 18], w int8 [Cout, 3, 3, cin_g], ws fp32 power-of-two classes, bias integers * 2^-4) and
    the statement's (s64, acc) of the lattice case (channels, pixels): shared by every test, read-only."""
    cin_g, cout_g, g = ch
    B, H, W = px
    r = X._rng("deform_conv_s8", ch, px)
    x = X.gen_int8(r, (B, H, W, cin_g * g))
    off = lattice_offsets(r, B, H, W)
    w, ws = X.gen_weights_int8(r, cout_g * g, TAPS * cin_g, True)
    w = w.reshape(cout_g * g, 3, 3, cin_g)
    bias = X.gen_bias(r, cout_g * g, "s8")
    s64 = column_s64(x, off)
    acc = sums(column(s64), w, g)
    for a in (x, off, w, ws, bias, s64, acc):
        a.setflags(write=False)
    return x, off, w, ws, bias, s64, acc


def lattice_statement(ch, px, full, relu, out):
    """-> (want, scale_out, t): every step of the epilogue asserted to be an fp32 number (power-of-two scales)."""
    x, off, w, ws, bias, s64, acc = lattice_case(ch, px)
    v = X.f32_exact(X.f32_exact(acc.astype(np.float64), "(float)sum") * (S_A * ws.astype(np.float64)), "* scale")
    if full:
        v = X.f32_exact(v + bias.astype(np.float64), "+ bias")
    if relu:
        v = np.maximum(v, 0.0)
    if out == "fp16":
        return v.astype(np.float32).astype(np.float16), 1.0, None
    s_out = 2.0 ** int(np.floor(np.log2(max(v.std(), 2.0 ** -20) / 48.0)))
    t = X.f32_exact(v / s_out, "/ scale_out")
    return np.clip(np.rint(t), -127, 127).astype(np.int8), s_out, t


GENERAL_SEEDS = (11, 12)


@functools.lru_cache(maxsize=None)
def general_case(ch, seed):
    """One-hot weights on Gaussian fp16 offsets at (2, 9, 15): output channel co of group g copies column byte
    (tap, ci) = KS[co] of its group.  -> (x, off, w, picks [Cout] of (tap, ci), s64 of the picked columns
    [B, H, W, Cout])."""
    cin_g, cout_g, g = ch
    B, H, W = PIXELS[1]
    r = X._rng("deform_conv_s8.general", ch, seed)
    x = X.gen_int8(r, (B, H, W, cin_g * g))
    off = general_offsets(r, B, H, W)
    w, picks = one_hot_weights(r, ch)
    s64 = column_s64(x, off)
    sel = np.stack([s64[..., t, (co // cout_g) * cin_g + ci] for co, (t, ci) in enumerate(picks)], axis=-1)
    for a in (x, off, w, sel):
        a.setflags(write=False)
    return x, off, w, picks, sel


def one_hot_weights(r, ch):
    """w int8 [Cout, 3, 3, cin_g] with ONE weight 1 per output channel at its own (tap, ci): every tap, the first and
    last channel of every tap and of every 16-byte vector among them -> (w, [(tap, ci)] per output channel)."""
    cin_g, cout_g, g = ch
    K = TAPS * cin_g
    must = sorted({t * cin_g for t in range(TAPS)} | {t * cin_g + cin_g - 1 for t in range(TAPS)} | {15, 16, 31, 32, K - 17})
    w = np.zeros((cout_g * g, TAPS, cin_g), np.int8)
    picks = []
    for grp in range(g):
        rest = [int(k) for k in r.permutation(K) if int(k) not in must]
        ks = (must[grp::g] + must + rest)[:cout_g] if g > 1 else (must + rest)[:cout_g]
        for c, k in enumerate(ks):
            t, ci = divmod(k, cin_g)
            w[grp * cout_g + c, t, ci] = 1
            picks.append((t, ci))
    return w.reshape(cout_g * g, 3, 3, cin_g), picks


GENERAL_S_A = 0.0173


def general_scale_operands(ch):
    """The lattice case (channels, 270 pixels) with per-channel weight scales and a bias that are no powers of two, and
    a scale_out from the statement's spread (values on both sides of the clamp) -> (w_scales, bias, scale_out)."""
    _, _, w, _, _, _, acc = lattice_case(ch, PIXELS[1])
    r = X._rng("deform_conv_s8.scales", ch)
    ws = (r.uniform(0.5, 2.0, size=w.shape[0]) * 3.1e-3).astype(np.float32)
    bias = r.normal(0.0, 0.3, size=w.shape[0]).astype(np.float32)
    v = acc * (float(np.float32(GENERAL_S_A)) * ws.astype(np.float64)) + bias
    return ws, bias, float(np.float32(v.std() / 40.0))
