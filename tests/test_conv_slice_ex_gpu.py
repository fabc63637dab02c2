"""bevops_conv_slice_f16_ex (csrc/conv_slice.hip): the dilated 3 x 3 convolution and the per-image bias of BEVDepth's
ASPP block, through the C ABI in the guarded arena of tests/util_arena.py under both poisons.

Every comparison is exact (tolerance 0): operands on the F16 lattice of tests/util_exact_dense.py (integers in [-8, 8]
* 2^-4, bias integers * 2^-6, identity integers * 2^-5; at most 9 * 96 products of at most 64 units of 2^-8, far below
2^24, so every fp32 partial sum is exact in any order) against a float64 statement of the dilated convolution: tap
(ky, kx) of output pixel (y, x) reads input pixel (y + (ky - 1) d, x + (kx - 1) d), zero outside the image.  Every byte
of the output buffer outside the slice must keep its poison bits and the guards must be intact."""
import functools

import numpy as np
import pytest
import torch

import util_exact_dense as X
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 16 << 20
NONE, RELU, SILU = 0, 1, 2


def _lib():
    from bevformer_tensorrt_amd.utils import lib as L
    return L, L.load_library(), L.current_stream_ptr(torch.device("cuda"))


def dconv64(x, w, d):
    """float64 [B, H, W, Cout] of the 3 x 3 (or 1 x 1) stride-1 convolution with dilation d, pad d * (k // 2)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, H, W, Cin = x.shape
    k = w.shape[1]
    p = d * (k // 2)
    xp = np.zeros((B, H + 2 * p, W + 2 * p, Cin))
    xp[:, p:p + H, p:p + W] = x
    out = np.zeros((B, H, W, w.shape[0]))
    for ky in range(k):
        for kx in range(k):
            out += xp[:, ky * d:ky * d + H, kx * d:kx * d + W] @ w[:, ky, kx].T
    return out


def _slice(arena, values, pitch, c0, name):
    B, H, W, C = values.shape
    buf = arena.empty((B, H, W, pitch), torch.float16, 16, name)
    view = buf[..., c0:c0 + C]
    view.copy_(torch.from_numpy(np.array(values)))
    return buf, view


def ex_call(arena, x, w, bias, res, act, dilation, xlay=(0, 0), olay=(0, 0), image_bias=None, bias_pitch=0, entry="ex"):
    """One call, every operand carved from `arena`.  xlay / olay = (extra pitch, first channel) of the x / out slice.
    image_bias [B, Cout] with bias_pitch >= Cout: the per-image rows.  entry "base": bevops_conv_slice_f16 (dilation 1,
    no per-image bias).  -> the out slice [B, H, W, Cout] as int16."""
    L, h, st = _lib()
    B, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    wd = arena.place(torch.from_numpy(np.array(w)), 16, "weight")
    bd = None
    if image_bias is not None:
        rows = np.zeros((B, bias_pitch), np.float16)
        rows[:, :Cout] = image_bias
        rows[:, Cout:] = np.float16(777.0)                # columns behind Cout are never read into the result
        bd = arena.place(torch.from_numpy(rows), 16, "image bias")
    elif bias is not None:
        bd = arena.place(torch.from_numpy(np.array(bias)), 2, "bias")
    xp, op = Cin + xlay[0], Cout + olay[0]
    _, xv = _slice(arena, x, xp, xlay[1], "x")
    obuf = arena.empty((B, H, W, op), torch.float16, 16, "out")
    ov = obuf[..., olay[1]:olay[1] + Cout]
    rv, rp = None, 0
    if res is not None:
        rp = Cout + 8
        _, rv = _slice(arena, res, rp, 0, "identity")
    before = obuf.cpu().numpy().view(np.uint8).copy()
    args = (xv.data_ptr(), xp, wd.data_ptr(), None if bd is None else bd.data_ptr(), None if rv is None else rv.data_ptr(),
            rp, ov.data_ptr(), op, B, H, W, Cin, Cout, k, 1, act)
    if entry == "base":
        assert dilation == 1 and image_bias is None
        rc = h.bevops_conv_slice_f16(*args, st)
    else:
        rc = h.bevops_conv_slice_f16_ex(*args, dilation, bias_pitch, st)
    assert rc == L.SUCCESS
    arena.check()
    after = obuf.cpu().numpy()
    mask = np.zeros(after.shape, bool)
    mask[..., olay[1]:olay[1] + Cout] = True
    mask8 = np.repeat(mask, 2, axis=-1)
    assert np.array_equal(after.view(np.uint8)[~mask8], before[~mask8]), "bytes outside the output slice were written"
    return after[..., olay[1]:olay[1] + Cout].copy().view(np.int16)


def both_poisons(*a, **kw):
    got = [ex_call(Arena(CAPACITY, poison), *a, **kw) for poison in POISONS]
    assert np.array_equal(got[0], got[1]), "results differ between the two poisons"
    return got[0]


def assert_bits(got, want):
    want = np.asarray(want).astype(np.float32).astype(np.float16)
    bad = np.argwhere(got != want.view(np.int16))
    assert len(bad) == 0, (f"{len(bad)} of {want.size} outputs differ, first at {tuple(bad[0])}: got "
                           f"{got.view(np.float16)[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")
    assert want.any()


# (B, H, W, Cin, Cout, dilation): 5 x 7 at dilation 6 -- every off-centre tap outside the image; R50's 16 x 44 map, two
# images, 1408 rows = 11 row tiles, the tile 640 .. 767 straddles the image boundary at row 704, 72 channels = the wide
# kernel with a partial column tile; a 3-pixel-wide image with three k-steps per tap and the narrow kernel
CASES = ((1, 5, 7, 32, 8, 6), (2, 16, 44, 32, 72, 6), (2, 16, 44, 32, 72, 12), (2, 16, 44, 32, 72, 18),
         (1, 19, 3, 96, 40, 2), (1, 13, 37, 64, 64, 12))


@functools.lru_cache(maxsize=None)
def lattice(case, k=3):
    B, H, W, Cin, Cout, d = case
    r = X._rng("conv_slice_ex", case, k)
    x, w = X.gen_f16_small(r, (B, H, W, Cin)), X.gen_f16_small(r, (Cout, k, k, Cin))
    bias = X.gen_bias(r, Cout, X.F16)
    res = X.gen_identity(r, (B, H, W, Cout), X.F16, "fp16")
    assert dconv64(np.abs(x), np.abs(w), d).max() * 2.0 ** 8 < 2.0 ** 24
    acc = X.f32_exact(dconv64(x, w, d), "sums")
    for a in (x, w, bias, res, acc):
        a.setflags(write=False)
    return x, w, bias, res, acc


@pytest.mark.parametrize("epi", ["plain", "bias+relu+identity"])
@pytest.mark.parametrize("case", CASES[:5], ids=lambda c: "x".join(map(str, c)))
def test_dilated_lattice_bits(case, epi):
    x, w, bias, res, acc = lattice(case)
    full = epi != "plain"
    if full:
        v = np.maximum(X.f32_exact(acc + bias.astype(np.float64), "+ bias"), 0.0)
        v = X.f32_exact(v + res.astype(np.float64), "+ identity")
    else:
        v = acc
    got = both_poisons(x, w, bias if full else None, res if full else None, RELU if full else NONE, case[5])
    assert_bits(got, v)


def test_off_centre_taps_of_the_5x7_case_are_outside_the_image():
    """5 x 7 at dilation 6 (the statement the case above is compared with): rows y +- 6 never exist, columns x +- 6 only
    for x = 0 and x = 6 -- in columns 1 .. 5 the result is the centre tap's 1 x 1 convolution, in the two border
    columns one more tap of the centre row."""
    x, w, _, _, acc = lattice(CASES[0])
    centre = dconv64(x, w[:, 1:2, 1:2], 1)
    assert np.array_equal(acc[:, :, 1:6], centre[:, :, 1:6])
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    assert np.array_equal(acc[:, :, 0], centre[:, :, 0] + x64[:, :, 6] @ w64[:, 1, 2].T)
    assert np.array_equal(acc[:, :, 6], centre[:, :, 6] + x64[:, :, 0] @ w64[:, 1, 0].T)


def test_pitched_input_into_slice_2_of_4():
    """x read from a slice with pitch Cin + 24 (at channel 8), out written into slice 2 of a 4-slice buffer: ASPP's
    concatenation buffer.  ex_call compares every byte outside the slice."""
    case = CASES[5]
    x, w, bias, _, acc = lattice(case)
    Cout = case[4]
    got = both_poisons(x, w, bias, None, RELU, case[5], xlay=(24, 8), olay=(3 * Cout, 2 * Cout))
    assert_bits(got, np.maximum(acc + bias.astype(np.float64), 0.0))


@pytest.mark.parametrize("d", [2, 6])
@pytest.mark.parametrize("y0,x0", [(0, 0), (12, 13), (6, 7), (6, 0), (3, 11)],
                         ids=["corner", "far-corner", "interior", "edge-left", "interior-odd"])
def test_one_hot_places_each_tap_at_its_dilated_offset(y0, x0, d):
    """x = 1 at one pixel, w[co, ky, kx, ci] = 2^(3 ky + kx - 8): output pixel (y0 - (ky - 1) d, x0 - (kx - 1) d) must
    hold the weight of tap (ky, kx), everything else zero."""
    B, H, W, Cin, Cout = 2, 13, 14, 32, 8
    x = np.zeros((B, H, W, Cin), np.float16)
    x[1, y0, x0, 5] = 1.0
    taps = 2.0 ** (3.0 * np.arange(3)[:, None] + np.arange(3)[None, :] - 8.0)
    w = np.broadcast_to(taps[None, :, :, None], (Cout, 3, 3, Cin)).astype(np.float16)
    want = np.zeros((B, H, W, Cout), np.float16)
    placed = 0
    for ky in range(3):
        for kx in range(3):
            yo, xo = y0 - (ky - 1) * d, x0 - (kx - 1) * d
            if 0 <= yo < H and 0 <= xo < W:
                want[1, yo, xo, :] = taps[ky, kx]
                placed += 1
    assert placed == (9 if (y0, x0) == (6, 7) else placed) and placed >= 4
    got = both_poisons(x, w, None, None, NONE, d).view(np.float16)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(want, dconv64(x, w, d).astype(np.float16))      # (the statement above is the convolution)


@pytest.mark.parametrize("k,d", [(1, 1), (3, 1), (3, 2)])
def test_image_bias_three_images_in_one_row_tile(k, d):
    """Three 5 x 7 images = 105 rows, all in ONE 128-row tile, three different bias rows of pitch Cout + 8: the image
    index is taken per row."""
    case = (3, 5, 7, 32, 72, d)
    x, w, _, res, acc = lattice(case, k)
    r = X._rng("image bias", k, d)
    ib = (r.integers(-256, 257, size=(3, 72)) * 2.0 ** -6).astype(np.float16)
    assert len({ib[b].tobytes() for b in range(3)}) == 3
    v = np.maximum(X.f32_exact(acc + ib.astype(np.float64)[:, None, None, :], "+ image bias"), 0.0)
    got = both_poisons(x, w, None, None, RELU, d, image_bias=ib, bias_pitch=80)
    assert_bits(got, v)
    # with an identity and a sliced output
    v2 = X.f32_exact(v + res.astype(np.float64), "+ identity")
    got = both_poisons(x, w, None, res, RELU, d, olay=(24, 16), image_bias=ib, bias_pitch=72)
    assert_bits(got, v2)


def test_image_bias_across_row_tiles_on_the_r50_map():
    case = CASES[1]
    x, w, _, _, acc = lattice(case)
    r = X._rng("image bias r50")
    ib = (r.integers(-256, 257, size=(2, 72)) * 2.0 ** -6).astype(np.float16)
    got = both_poisons(x, w, None, None, NONE, case[5], image_bias=ib, bias_pitch=72)
    assert_bits(got, acc + ib.astype(np.float64)[:, None, None, :])


# (B, H, W, Cin, Cout, k, with identity, act): three shapes of tests/test_conv_slice_gpu.py
SAME = ((3, 7, 9, 96, 64, 3, True, RELU), (1, 11, 12, 96, 136, 3, True, SILU), (1, 9, 14, 512, 8, 1, False, SILU))


@pytest.mark.parametrize("geom", SAME, ids=lambda g: "x".join(map(str, g)))
def test_dilation_1_without_image_bias_is_the_parent_entry_bit_for_bit(geom):
    B, H, W, Cin, Cout, k, with_res, act = geom
    r = X._rng("conv_slice_ex vs base", geom)
    x = r.standard_normal((B, H, W, Cin)).astype(np.float16)
    w = (2.0 * r.standard_normal((Cout, k, k, Cin)) / np.sqrt(k * k * Cin)).astype(np.float16)
    bias = (0.5 * r.standard_normal(Cout)).astype(np.float16)
    res = r.standard_normal((B, H, W, Cout)).astype(np.float16) if with_res else None
    lay = dict(xlay=(40, 8), olay=(24, 16))
    a = both_poisons(x, w, bias, res, act, 1, entry="ex", **lay)
    b = both_poisons(x, w, bias, res, act, 1, entry="base", **lay)
    assert np.array_equal(a, b) and a.any()


def test_a_nan_input_reaches_exactly_the_outputs_whose_taps_read_it():
    case = CASES[1]
    B, H, W, Cin, Cout, d = case
    x, w, bias, _, _ = lattice(case)
    w = np.where(w == 0, np.float16(2.0 ** -4), w)                # every tap of every channel multiplies the NaN
    clean = both_poisons(x, w, bias, None, NONE, d)
    b0, y0, x0 = 1, 3, 40
    xi = x.copy()
    xi[b0, y0, x0, 17] = np.nan
    got = both_poisons(xi, w, bias, None, NONE, d).view(np.float16)
    reached = np.zeros((B, H, W), bool)
    for ky in range(3):
        for kx in range(3):
            yo, xo = y0 - (ky - 1) * d, x0 - (kx - 1) * d
            if 0 <= yo < H and 0 <= xo < W:
                reached[b0, yo, xo] = True
    assert reached.sum() == 4                                     # rows 3, 9 x columns 34, 40 (46 and -3 are outside)
    nan = np.isnan(got)
    assert nan[reached].all(), "an output whose tap reads the NaN is a number"
    assert not nan[~reached].any()
    assert np.array_equal(got.view(np.int16)[~reached], clean[~reached])


def test_wrapper_dilation_and_image_bias():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.functions import yolox_ops as Y
    case = (3, 5, 7, 32, 72, 2)
    x, w, _, _, acc = lattice(case, 3)
    r = X._rng("wrapper image bias")
    ib = (r.integers(-256, 257, size=(3, 72)) * 2.0 ** -6).astype(np.float16)
    want = np.maximum(acc + ib.astype(np.float64)[:, None, None, :], 0.0).astype(np.float32).astype(np.float16)
    wt = torch.from_numpy(w.copy()).cuda().permute(0, 3, 1, 2).contiguous()
    xs = Y.nhwc_empty(3, 32, 5, 7, "cuda")
    xs.copy_(torch.from_numpy(x.copy()).cuda().permute(0, 3, 1, 2))
    buf = Y.nhwc_empty(3, 4 * 72, 5, 7, "cuda")
    buf.fill_(float("nan"))
    y = bev.conv_slice_nhwc(xs, wt, None, "relu", out=buf[:, 72:144], dilation=2, image_bias=torch.from_numpy(ib).cuda())
    assert np.array_equal(y.permute(0, 2, 3, 1).cpu().numpy().view(np.int16), want.view(np.int16))
    assert torch.isnan(buf[:, :72]).all() and torch.isnan(buf[:, 144:]).all()
    from bevformer_tensorrt_amd.utils.lib import BevopsError, NOT_SUPPORTED
    with pytest.raises(BevopsError) as e:
        bev.conv_slice_nhwc(xs, wt, None, "relu", stride=2, dilation=2)
    assert e.value.status == NOT_SUPPORTED
    with pytest.raises(ValueError, match="one of them"):
        bev.conv_slice_nhwc(xs, wt, torch.zeros(72, device="cuda", dtype=torch.float16), "relu", dilation=2,
                            image_bias=torch.from_numpy(ib).cuda())
