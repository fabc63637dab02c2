"""bevops_dwsep_conv_s8 (csrc/dwsep_conv_s8.hip) through functions.yolox_ops.dwsep_conv_q_taps in the guarded arena of
tests/util_arena.py, against the statement of the operation order in include/bevops.h.  The launch is bevops_conv_slice_s8's
epilogue twice: stage 1 on the exact depthwise sums with (scale_a, scale_w, scale_out) = (scale_x, 1, scale_t), stage 2 on
the exact pointwise sums of the bytes t with scale_a = scale_t -- so tests/util_conv_slice_s8.py states both
(`exact_output`: the fp32 operations evaluated in the extended type; `silu_interval` / `check_interval`).
Exact tests: x_q, w_dw_q, w_pw_q integers in [-8, 8], power-of-two scales, biases on the grid of the products:
|sum_dw| <= 576, |sum_pw| <= 160 * 127 * 8 < 2^24, every fp32 step exact; scale_t = 2 scale_x w_dw_scale puts t = sum_dw / 2
+ ... on half-integers for odd sums (ties to even) and beyond +-127.  design/yolox_depthwise_int8.md derives the bounds."""
import functools

import numpy as np
import pytest
import torch

import util_conv_slice_s8 as S
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu
ACT = {"none": 0, "relu": 1, "silu": 2}


def dw_sums(x, wd, stride):
    """int64 [B, Ho, Wo, C]: x int8 [B, H, W, C], wd [3, 3, C], pad 1."""
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 2, W + 2, C), np.int64)
    xp[:, 1:-1, 1:-1] = x
    return sum(xp[:, ky:ky + H:stride, kx:kx + W:stride] * wd[ky, kx].astype(np.int64) for ky in range(3) for kx in range(3))


def launch(poison, o, out_kind="int8"):
    """One call in a fresh arena: x, identity and out are channels 16 .. of buffers 48 / 32 / 32 channels wider.
    o: numpy operands (x [B, H, W, C], wd, sd, bd, wp, sp, bp, res, scalars, acts, stride).  -> out [B, Ho, Wo, Co]."""
    from bevformer_tensorrt_amd.functions import dwsep_conv_q_taps
    A = Arena(8 << 20, poison)
    (B, H, W, C), Co, s = o["x"].shape, o["wp"].shape[0], o["stride"]
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    dt = torch.int8 if out_kind == "int8" else torch.float16
    xs = A.empty((B, C + 48, H, W), torch.int8, 16, "x", channels_last=True)[:, 16:16 + C]
    xs.copy_(torch.from_numpy(o["x"]).permute(0, 3, 1, 2))
    obuf = A.empty((B, Co + 32, Ho, Wo), dt, 16, "out", channels_last=True)
    out, rs = obuf[:, 16:16 + Co], None
    if o.get("res") is not None:
        rs = A.empty((B, Co + 32, Ho, Wo), torch.int8, 16, "identity", channels_last=True)[:, 16:16 + Co]
        rs.copy_(torch.from_numpy(o["res"]).permute(0, 3, 1, 2))
    dev = lambda k, align=16: None if o.get(k) is None else A.place(torch.from_numpy(o[k]), align, k)      # noqa: E731
    before = obuf.clone()
    got = dwsep_conv_q_taps(xs, o["sx"], dev("wd"), dev("sd"), dev("bd"), o["st"], dev("wp"), dev("sp", 4), dev("bp", 4),
                            o["acts"][0], o["acts"][1], rs, o.get("sr", 1.0), s, out, o.get("so"), dt)
    A.check()
    other = torch.ones(obuf.shape[1], dtype=torch.bool)
    other[16:16 + Co] = False
    assert torch.equal(obuf[:, other].cpu().view(torch.uint8), before[:, other].cpu().view(torch.uint8)), \
        "bytes outside the output slice were written"
    return got.permute(0, 2, 3, 1).contiguous().cpu().numpy()


def both_poisons(o, out_kind="int8"):
    a, b = (launch(p, o, out_kind) for p in POISONS)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "results differ between the two poisons"
    return a


def stage1(o):
    """(sum_dw, t int8) of the exact statement (act none / ReLU)."""
    acc = dw_sums(o["x"], o["wd"], o["stride"])
    return acc, S.exact_output(acc, o["sx"], 1.0, o["sd"], o.get("bd"), ACT[o["acts"][0]], None, 1.0, o["st"], "int8")


def stage2_sums(t, wp):
    return t.astype(np.int64) @ wp.astype(np.int64).T


def statement(o, out_kind="int8", t=None):
    t = stage1(o)[1] if t is None else t
    return S.exact_output(stage2_sums(t, o["wp"]), o["st"], 1.0, o["sp"], o.get("bp"), ACT[o["acts"][1]], o.get("res"),
                          o.get("sr", 1.0), o.get("so"), out_kind)


@functools.lru_cache(maxsize=None)
def lattice(B, H, W, C, Co, stride):
    r = np.random.default_rng(1000 * C + 10 * Co + H)
    i8 = lambda *s: r.integers(-8, 9, size=s).astype(np.int8)                                         # noqa: E731
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return dict(x=i8(B, H, W, C), wd=i8(3, 3, C), wp=i8(Co, C), stride=stride,
                sx=2.0 ** -2, sd=np.full(C, 2.0 ** -2, np.float32), st=2.0 ** -3,       # t = sum_dw / 2 + 8 bias_dw
                sp=np.full(Co, 2.0 ** -6, np.float32), sr=2.0 ** -2, so=2.0 ** -4,      # v2 on the grid 2^-9
                bd=(r.integers(-512, 513, size=C) * 2.0 ** -4).astype(np.float32),
                bp=(r.integers(-256, 257, size=Co) * 2.0 ** -9).astype(np.float32),
                res=r.integers(-127, 128, size=(B, Ho, Wo, Co)).astype(np.int8))


# (B, H, W, Cin, Cout, stride): one pixel, half-empty step, narrow tile | 1.5 steps, two images in a tile, four borders |
# two row and two column tiles with ragged seconds | stride 2 on odd sizes, 2.5 steps | stride 2, even steps
SHAPES = ((1, 1, 1, 32, 16, 1), (2, 5, 7, 96, 64, 1), (1, 12, 13, 64, 144, 1), (2, 7, 9, 160, 48, 2), (1, 9, 8, 128, 128, 2))


@pytest.mark.parametrize("out_kind", ["int8", "fp16"])
@pytest.mark.parametrize("plain", [False, True], ids=["bias+identity", "plain"])
@pytest.mark.parametrize("acts", [("none", "none"), ("relu", "relu"), ("relu", "none")], ids="-".join)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_exact_bytes(shape, acts, plain, out_kind):
    o = dict(lattice(*shape), acts=acts)
    if plain:
        o.update(bd=None, bp=None, res=None)
    acc, t = stage1(o)
    tr = acc.astype(np.float64) / 2 + (0 if plain else 8 * o["bd"])
    assert np.abs(acc).max() <= 576 and (plain or (np.abs(tr) > 127).any())                          # beyond the clamp
    assert (np.abs(tr - np.floor(tr)) == 0.5).any()                                                  # ties to even
    want = statement(o, out_kind, t)
    got = both_poisons(o, out_kind)
    assert got.dtype == want.dtype and want.any()
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{int((got != want).sum())} outputs differ"


def eye_layer(x, wd, stride, acts=("none", "none"), **kw):
    """Cout = Cin with the identity pointwise weight and scale_out = scale_t: the output is t, byte for byte."""
    C = x.shape[-1]
    o = dict(x=x, wd=wd, wp=np.eye(C, dtype=np.int8), stride=stride, sx=1.0, sd=np.ones(C, np.float32), st=1.0,
             sp=np.ones(C, np.float32), so=1.0, acts=acts)
    o.update(kw)
    o["so"] = o["st"]
    return o


@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("tap", range(9))
def test_one_hot_tap_moves_its_pixel(tap, stride, C):
    B, H, W, ky, kx = 2, 5, 6, tap // 3, tap % 3
    x = ((np.arange(B * H * W).reshape(B, H, W, 1) * 7 + np.arange(C) * 3) % 251 - 125).astype(np.int8)
    wd = np.zeros((3, 3, C), np.int8)
    wd[ky, kx] = 1
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    want = np.zeros((B, Ho, Wo, C), np.int8)
    for yo in range(Ho):
        for xo in range(Wo):
            y, xx = stride * yo + ky - 1, stride * xo + kx - 1
            if 0 <= y < H and 0 <= xx < W:
                want[:, yo, xo] = x[:, y, xx]
    assert np.array_equal(both_poisons(eye_layer(x, wd, stride)), want) and want.any()


def stage1_interval(acc, sx, sd, bd, st):
    """silu_interval for stage 1's own order: sc = f32(scale_x w_dw_scales[c]) is ONE rounding and (float)sum_dw is exact
    (util_conv_slice_s8's order has three roundings in front of the fma), so with P = |sum_dw| sc:
    e_v = u (P + |v|)(1 + 2^-20); SiLU as there: e_a = 1.1 e_v + 2^-17 (|silu v| + 1.1 e_v) + 2^-120; no identity;
    delta = (e_a (1 + 3 u) + 2.01 u |silu v|) / scale_t  (inv_t's rounding and the product's)."""
    sc = float(np.float32(sx)) * sd.astype(np.float64)
    prod = acc.astype(np.float64) * sc
    v = prod + bd.astype(np.float64)
    a = S.silu64(v)
    e_v = S.U * (np.abs(prod) + np.abs(v)) * (1.0 + 2.0 ** -20)
    e_a = 1.1 * e_v + 2.0 ** -17 * (np.abs(a) + 1.1 * e_v) + 2.0 ** -120
    st = float(np.float32(st))
    delta = (e_a * (1.0 + 3.0 * S.U) + 2.01 * S.U * np.abs(a)) / st
    q = lambda z: np.clip(np.rint(z), -127, 127).astype(np.int8)                                      # noqa: E731
    return q(a / st - delta), q(a / st + delta)


@pytest.mark.parametrize("geom", [(2, 7, 9, 96, 2), (1, 12, 13, 160, 1)], ids=lambda g: "x".join(map(str, g)))
def test_stage1_silu_is_observable_and_inside_its_interval(geom):
    B, H, W, C, stride = geom
    r = np.random.default_rng(C + H)
    gauss = lambda *s: np.clip(np.rint(r.normal(0, 40, size=s)), -127, 127).astype(np.int8)           # noqa: E731
    sd = (r.uniform(0.5, 1.5, size=C) * 1.7e-2).astype(np.float32)
    bd = r.normal(0, 0.5, size=C).astype(np.float32)
    o = eye_layer(gauss(B, H, W, C), gauss(3, 3, C), stride, ("silu", "none"), sx=0.0371, sd=sd, bd=bd, st=0.0473)
    acc = dw_sums(o["x"], o["wd"], stride)
    lo, hi = stage1_interval(acc, o["sx"], sd, bd, o["st"])
    f = np.float32                                    # the statement in float32 on the CPU stays inside the cap too
    v32 = acc.astype(f) * (f(o["sx"]) * sd) + bd
    t32 = np.clip(np.rint(v32 / (f(1) + np.exp(-v32)) * (f(1) / f(o["st"]))), -127, 127).astype(np.int8)
    S.check_interval(t32, lo, hi)
    got = both_poisons(o)
    share = S.check_interval(got, lo, hi)
    print(f"stage-1 SiLU {geom}: {share:.4%} of the outputs within delta of a half-integer, "
          f"{float((np.abs(got) == 127).mean()):.2%} clamped")
    assert len(np.unique(got)) > 100


@pytest.mark.parametrize("shape", [(2, 7, 9, 96, 48, 2), (1, 12, 13, 64, 144, 1)], ids=lambda c: "x".join(map(str, c)))
def test_stage2_silu_inside_the_interval_of_the_slice_convolution(shape):
    o = dict(lattice(*shape), acts=("relu", "silu"))
    r = np.random.default_rng(shape[4])
    o.update(sp=(r.uniform(0.5, 1.5, size=shape[4]) * 0.011).astype(np.float32), so=0.0437, sr=0.0291,
             bp=r.normal(0, 0.5, size=shape[4]).astype(np.float32))
    acc2 = stage2_sums(stage1(o)[1], o["wp"])
    _, _, lo, hi = S.silu_interval(acc2, o["st"], 1.0, o["sp"], o["bp"], o["res"], o["sr"], o["so"])
    got = both_poisons(o)
    print(f"stage-2 SiLU {shape}: {S.check_interval(got, lo, hi):.4%} within delta of a half-integer")
    assert len(np.unique(got)) > 100


@pytest.mark.parametrize("shape", [(2, 5, 7, 96, 64, 1), (1, 12, 13, 64, 144, 1)], ids=["narrow", "wide"])
def test_equals_the_two_launch_form_bit_for_bit(shape):
    """bevops_conv_slice_s8 (1 x 1) on the statement's t bytes, general pointwise scales and SiLU behind it."""
    from bevformer_tensorrt_amd.functions import conv_slice_q_taps
    o = dict(lattice(*shape), acts=("relu", "silu"))
    r = np.random.default_rng(7)
    o.update(sp=(r.uniform(0.5, 1.5, size=shape[4]) * 0.011).astype(np.float32), so=0.0137, sr=0.0291)
    t = stage1(o)[1]
    cuda = lambda a: torch.from_numpy(a).cuda()                                                       # noqa: E731
    nhwc = lambda a: cuda(a).permute(0, 3, 1, 2)                                                      # noqa: E731
    two = conv_slice_q_taps(nhwc(t), o["st"], cuda(o["wp"]).view(shape[4], 1, 1, shape[3]), cuda(o["sp"]), cuda(o["bp"]),
                            "silu", nhwc(o["res"]), o["sr"], 1, None, o["so"])
    assert np.array_equal(both_poisons(o), two.permute(0, 2, 3, 1).cpu().numpy())


def test_a_nan_bias_stays_in_its_channel_or_its_column():
    o = dict(lattice(2, 7, 9, 160, 48, 2), acts=("none", "none"))
    c, co = int(np.argmin(np.abs(o["bd"]))), 21       # a channel whose finite t is not clamped already
    o["wp"] = o["wp"].copy()
    o["wp"][::5, c] = 0                               # outputs channel c cannot reach
    clean, t = both_poisons(o), stage1(o)[1]
    bd = o["bd"].copy()
    bd[c] = np.nan
    t[..., c] = -127                                  # max(NaN, -127): the channel's t, reaching column c of w_pw alone
    got = both_poisons(dict(o, bd=bd))
    assert np.array_equal(got, statement(o, "int8", t))
    reach = o["wp"][:, c] != 0
    assert np.array_equal(got[..., ~reach], clean[..., ~reach]) and (~reach).any() and (got != clean).any()
    bp = o["bp"].copy()
    bp[co] = np.nan
    got = both_poisons(dict(o, bp=bp))
    keep = np.arange(48) != co
    assert np.array_equal(got[..., keep], clean[..., keep]) and (got[..., co] == -127).all()
