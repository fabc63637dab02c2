"""bevops_conv_slice_f16 (csrc/conv_slice.hip) through the C ABI in the guarded arena of tests/util_arena.py.

Exact tests (tolerance 0): operands on the F16 lattice of tests/util_exact_dense.py (integers in [-8, 8] * 2^-4, bias
integers * 2^-6, identity integers * 2^-5; a sum has at most 9 * 512 products of at most 64 units of 2^-8, far below
2^24, so every fp32 partial sum is exact in any order), act in {none, ReLU}, against a float64 convolution on the CPU;
the operands as channel slices of wider buffers (x_pitch = Cin + 40 at channel 8, out_pitch = Cout + 24 at channel 16,
res_pitch = Cout + 8), dense, or x and out as two slices of ONE buffer.  Every byte of the output buffer outside the
slice must keep its poison bits, the guards must be intact, and the two poisons must give equal bits.

SiLU: |got - e| <= 2^-11 |e| + 2^-17 |silu64(s)| + 2^-25 with s the exact sum + bias and e = silu64(s) + identity: one
fp16 rounding, half a subnormal step, and the fp32 evaluation of v * rcp(1 + exp(-v)) with the hardware exponential
(|v| 2^-24 relative from the scaled argument below |v| = 88, a few 2^-24 for exp, add, reciprocal, multiply and the
identity add: under 128 * 2^-24 = 2^-17 together; beyond 88 the result saturates to -0 or v).  Derived, not measured; the
measured maximum is printed as a fraction of the bound.  On Gaussian operands the accumulation term of
tests/test_deconv_gpu.py, (K + 1) 2^-24 sum |x w|, is added."""
import functools

import numpy as np
import pytest
import torch

import util_exact_dense as X
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 24 << 20
NONE, RELU, SILU = 0, 1, 2


def _lib():
    from bevformer_tensorrt_amd.utils import lib as L
    return L, L.load_library(), L.current_stream_ptr(torch.device("cuda"))


def _place_slice(arena, values, pitch, c0, name):
    """values [B, H, W, C] fp16 as channels c0 .. c0 + C of a poisoned [B, H, W, pitch] buffer -> (buffer, slice view)."""
    B, H, W, C = values.shape
    buf = arena.empty((B, H, W, pitch), torch.float16, 16, name)
    view = buf[..., c0:c0 + C]
    view.copy_(torch.from_numpy(np.array(values)))
    return buf, view


def c_call(arena, x, w, bias, res, act, stride, layout):
    """One call with every operand carved from `arena`.  layout 'slice': x, identity and out are channel slices of
    wider buffers; 'dense': pitch == channels; 'same': x and out are disjoint slices of ONE buffer (stride 1).
    -> (out slice [B, Ho, Wo, Cout] as a host int16 array, host copy of the whole output buffer as bytes, slice mask)."""
    L, h, st = _lib()
    B, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    Ho, Wo = X.conv_out_hw(H, W, k, stride)
    wd = arena.place(torch.from_numpy(np.array(w)), 16, "weight")
    bd = None if bias is None else arena.place(torch.from_numpy(np.array(bias)), 2, "bias")
    if layout == "same":
        assert stride == 1
        pitch = Cin + Cout + 8
        buf, xv = _place_slice(arena, x, pitch, 0, "x|out")
        obuf, oc0, op, xp = buf, Cin, pitch, pitch
    else:
        xp, xc0 = (Cin, 0) if layout == "dense" else (Cin + 40, 8)
        op, oc0 = (Cout, 0) if layout == "dense" else (Cout + 24, 16)
        _, xv = _place_slice(arena, x, xp, xc0, "x")
        obuf = arena.empty((B, Ho, Wo, op), torch.float16, 16, "out")
    ov = obuf[..., oc0:oc0 + Cout]
    rv, rp = None, 0
    if res is not None:
        rp = Cout if layout == "dense" else Cout + 8
        _, rv = _place_slice(arena, res, rp, 0, "identity")
    before = obuf.cpu().numpy().view(np.uint8).copy()
    rc = h.bevops_conv_slice_f16(xv.data_ptr(), xp, wd.data_ptr(), None if bd is None else bd.data_ptr(),
                                 None if rv is None else rv.data_ptr(), rp, ov.data_ptr(), op, B, H, W, Cin, Cout, k,
                                 stride, act, st)
    assert rc == L.SUCCESS
    arena.check()
    after = obuf.cpu().numpy()
    mask = np.zeros(after.shape, bool)
    mask[..., oc0:oc0 + Cout] = True
    mask8 = np.repeat(mask, 2, axis=-1)
    a8 = after.view(np.uint8)
    assert np.array_equal(a8[~mask8], before[~mask8]), "bytes of the output buffer outside the slice were written"
    return after[..., oc0:oc0 + Cout].copy().view(np.int16)


def run_both_poisons(x, w, bias, res, act, stride, layout):
    got = [c_call(Arena(CAPACITY, poison), x, w, bias, res, act, stride, layout) for poison in POISONS]
    assert np.array_equal(got[0], got[1]), "results differ between the two poisons"
    return got[0]


def _conv64(x, w, k, stride):
    """exact float64 sums [B, Ho, Wo, Cout]"""
    B, H, W, _ = x.shape
    Ho, Wo = X.conv_out_hw(H, W, k, stride)
    return X.int_conv(x, w, k, stride).reshape(B, Ho, Wo, w.shape[0])


# ---------------------------------------------------------------------------------------------- tolerance 0
# (B, H, W, Cin, Cout, ksize, stride, layout): images 1 x 1, 7 x 9, 9 x 14 (126 rows, one short of a tile), 11 x 12 (132
# rows, across a tile edge); Cin 32, 96 (three steps per tap), 512; Cout 8, 64, 96, 136 (across a column-tile edge)
CASES = ((1, 1, 1, 32, 8, 1, 1, "dense"), (1, 1, 1, 32, 8, 3, 2, "slice"), (3, 7, 9, 96, 64, 3, 2, "slice"),
         (3, 7, 9, 32, 136, 3, 1, "slice"), (3, 7, 9, 96, 64, 1, 2, "dense"), (1, 9, 14, 96, 96, 3, 1, "slice"),
         (1, 9, 14, 512, 8, 1, 1, "dense"), (1, 11, 12, 32, 64, 3, 1, "same"), (1, 11, 12, 96, 136, 1, 2, "slice"),
         (1, 11, 12, 96, 136, 3, 1, "same"), (3, 11, 12, 512, 96, 3, 2, "dense"), (3, 9, 14, 32, 96, 1, 1, "same"))


@functools.lru_cache(maxsize=None)
def lattice_case(case):
    B, H, W, Cin, Cout, k, stride, _ = case
    r = X._rng("conv_slice", case)
    x, w = X.gen_f16_small(r, (B, H, W, Cin)), X.gen_f16_small(r, (Cout, k, k, Cin))
    bias = X.gen_bias(r, Cout, X.F16)
    Ho, Wo = X.conv_out_hw(H, W, k, stride)
    res = X.gen_identity(r, (B, Ho, Wo, Cout), X.F16, "fp16")
    worst = X.int_conv(np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64)), k, stride).max()
    assert worst * 2.0 ** 8 < 2.0 ** 24
    acc = X.f32_exact(_conv64(x, w, k, stride), "sums")
    for a in (x, w, bias, res, acc):
        a.setflags(write=False)
    return x, w, bias, res, acc


@pytest.mark.parametrize("act", [NONE, RELU], ids=["linear", "relu"])
@pytest.mark.parametrize("epi", ["plain", "bias+identity"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_lattice_bits(case, epi, act):
    x, w, bias, res, acc = lattice_case(case)
    full = epi != "plain"
    v = X.f32_exact(acc + bias.astype(np.float64), "+ bias") if full else acc
    v = np.maximum(v, 0.0) if act == RELU else v
    if full:
        v = X.f32_exact(v + res.astype(np.float64), "+ identity")        # the identity AFTER the activation
    want = v.astype(np.float32).astype(np.float16)                        # the ONE rounding
    got = run_both_poisons(x, w, bias if full else None, res if full else None, act, case[6], case[7])
    bad = np.argwhere(got != want.view(np.int16))
    assert len(bad) == 0, (f"{len(bad)} of {want.size} outputs differ, first at {tuple(bad[0])}: got "
                           f"{got.view(np.float16)[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")
    assert want.any()


def test_the_identity_is_added_after_the_activation():
    """conv = -1 and identity = +2 with ReLU: relu(-1) + 2 = 2, not relu(-1 + 2) = 1."""
    B, H, W, Cin, Cout = 1, 3, 5, 32, 8
    x = np.ones((B, H, W, Cin), np.float16)
    w = np.zeros((Cout, 1, 1, Cin), np.float16)
    w[:, 0, 0, 3] = -1.0
    res = np.full((B, H, W, Cout), 2.0, np.float16)
    got = run_both_poisons(x, w, None, res, RELU, 1, "slice").view(np.float16)
    assert np.all(got == 2.0), np.unique(got)
    got = run_both_poisons(x, w, None, res, NONE, 1, "slice").view(np.float16)
    assert np.all(got == 1.0)


# ---------------------------------------------------------------------------------------------- which tap lands where
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("y0,x0", [(0, 0), (4, 5), (0, 3), (2, 0), (2, 3), (3, 2)],
                         ids=["corner", "far-corner", "edge-top", "edge-left", "interior", "interior-odd"])
def test_one_hot_names_its_tap(y0, x0, stride):
    """x = 1 at one pixel and channel, w[co, ky, kx, ci] = 2^(3 ky + kx - 8): output pixel (yo, xo) must hold the weight
    of tap (ky, kx) = (y0 - s yo + 1, x0 - s xo + 1) when that is a tap, and zero otherwise."""
    B, H, W, Cin, Cout, c0 = 2, 5, 6, 32, 8, 5
    x = np.zeros((B, H, W, Cin), np.float16)
    x[1, y0, x0, c0] = 1.0
    taps = 2.0 ** (3.0 * np.arange(3)[:, None] + np.arange(3)[None, :] - 8.0)
    w = np.broadcast_to(taps[None, :, :, None], (Cout, 3, 3, Cin)).astype(np.float16)
    Ho, Wo = X.conv_out_hw(H, W, 3, stride)
    want = np.zeros((B, Ho, Wo, Cout), np.float16)
    for yo in range(Ho):
        for xo in range(Wo):
            ky, kx = y0 - stride * yo + 1, x0 - stride * xo + 1
            if 0 <= ky < 3 and 0 <= kx < 3:
                want[1, yo, xo, :] = taps[ky, kx]
    got = run_both_poisons(x, w, None, None, NONE, stride, "slice").view(np.float16)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(want, _conv64(x, w, 3, stride).astype(np.float16))      # (the statement above is conv2d)


# ---------------------------------------------------------------------------------------------- non-finite containment
@pytest.mark.parametrize("stride", [1, 2])
def test_an_infinite_input_reaches_its_receptive_field_only(stride):
    case = (3, 7, 9, 96, 64, 3, stride, "slice")
    B, H, W, Cin, Cout, k, _, layout = case
    x, w, bias, res, _ = lattice_case(case)
    clean = run_both_poisons(x, w, bias, res, NONE, stride, layout)
    b0, y0, x0 = 1, 3, 4
    xi = x.copy()
    xi[b0, y0, x0, 17] = np.inf
    got = run_both_poisons(xi, w, bias, res, NONE, stride, layout)
    Ho, Wo = X.conv_out_hw(H, W, k, stride)
    reached = np.zeros((B, Ho, Wo), bool)
    for yo in range(Ho):
        for xo in range(Wo):
            reached[b0, yo, xo] = abs(stride * yo - y0) <= 1 and abs(stride * xo - x0) <= 1
    assert reached.sum() == (9 if stride == 1 else 2)        # (stride 2: rows 1 and 2 see y0 = 3 -> 2 x 1 with x0 = 4)
    finite = np.isfinite(got.view(np.float16))
    assert not finite[reached].any(), "an output whose window holds the infinite input is finite"
    assert finite[~reached].all()
    assert np.array_equal(got[~reached], clean[~reached])


# ---------------------------------------------------------------------------------------------- SiLU
def silu64(s):
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(over="ignore"):
        return s / (1.0 + np.exp(-s))


def silu_bound(s, e):
    return 2.0 ** -11 * np.abs(e) + 2.0 ** -17 * np.abs(silu64(s)) + 2.0 ** -25


@pytest.mark.parametrize("with_res", [False, True], ids=["noidentity", "identity"])
def test_silu_on_the_lattice_sweeps_the_argument(with_res):
    """s = exact sum + bias with the bias sweeping [-20, 20] in steps of 5 / 16 and the saturating tails beyond
    |v| = 88; 136 output channels."""
    B, H, W, Cin, Cout = 1, 9, 14, 32, 136
    r = X._rng("conv_slice silu sweep")
    x, w = X.gen_f16_small(r, (B, H, W, Cin)), X.gen_f16_small(r, (Cout, 1, 1, Cin))
    bias = np.concatenate([-20.0 + 0.3125 * np.arange(129), [-120.0, -100.0, -89.0, -88.5, 88.5, 89.0, 100.0]])
    assert bias.size == Cout and np.array_equal(bias.astype(np.float16).astype(np.float64), bias)
    res = X.gen_identity(r, (B, H, W, Cout), X.F16, "fp16") if with_res else None
    s = X.f32_exact(_conv64(x, w, 1, 1) + bias, "sum + bias")
    assert s.min() < -88 and s.max() > 88 and ((s > -20) & (s < 20)).mean() > 0.8
    e = silu64(s) + (res.astype(np.float64) if with_res else 0.0)
    got = run_both_poisons(x, w, bias.astype(np.float16), res, SILU, 1, "slice").view(np.float16).astype(np.float64)
    assert np.isfinite(got).all()
    err, bound = np.abs(got - e), silu_bound(s, e)
    print(f"SiLU lattice sweep, identity {with_res}: max |err| {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"{int((err > bound).sum())} outputs beyond the bound, worst ratio {np.max(err / bound):.3f}"


# three YOLOX-x layer geometries, spatially shrunk: the stage-2 down-sample 160 -> 320 3x3 / 2, a stage-2 bottleneck's
# second convolution 160 -> 160 3x3 with the identity, a top-down CSP layer's final 1x1 640 -> 640
GAUSSIAN = ((1, 16, 16, 160, 320, 3, 2, False), (2, 16, 13, 160, 160, 3, 1, True), (1, 12, 12, 640, 640, 1, 1, False))


@pytest.mark.parametrize("geom", GAUSSIAN, ids=lambda g: "x".join(map(str, g[:7])))
def test_silu_on_gaussian_operands_within_the_accumulation_bound(geom):
    B, H, W, Cin, Cout, k, stride, with_res = geom
    r = X._rng("conv_slice gaussian", geom)
    x = r.standard_normal((B, H, W, Cin)).astype(np.float16)
    w = (2.0 * r.standard_normal((Cout, k, k, Cin)) / np.sqrt(k * k * Cin)).astype(np.float16)
    bias = (0.5 * r.standard_normal(Cout)).astype(np.float16)
    Ho, Wo = X.conv_out_hw(H, W, k, stride)
    res = r.standard_normal((B, Ho, Wo, Cout)).astype(np.float16) if with_res else None
    s = _conv64(x, w, k, stride) + bias.astype(np.float64)
    mag = _conv64(np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64)), k, stride)
    e = silu64(s) + (res.astype(np.float64) if with_res else 0.0)
    K = k * k * Cin
    bound = silu_bound(s, e) + (K + 1) * 2.0 ** -24 * mag
    got = run_both_poisons(x, w, bias, res, SILU, stride, "slice").view(np.float16).astype(np.float64)
    err = np.abs(got - e)
    print(f"SiLU Gaussian {geom}: max |err| {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"{int((err > bound).sum())} outputs beyond the bound, worst ratio {np.max(err / bound):.3f}"


# ---------------------------------------------------------------------------------------------- against the existing kernel
@pytest.mark.parametrize("act", [NONE, RELU], ids=["linear", "relu"])
@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 1), (1, 2)])
def test_dense_call_equals_conv_tile_bit_for_bit(k, stride, act):
    """pitch == channels, no identity: the k-order and the MFMA sequence are bevops_conv_tile_f16's."""
    L, h, st = _lib()
    B, H, W, Cin, Cout = 2, 11, 13, 96, 136
    r = X._rng("conv_slice vs conv_tile", k, stride)
    x = r.standard_normal((B, H, W, Cin)).astype(np.float16)
    w = (r.standard_normal((Cout, k, k, Cin)) / np.sqrt(k * k * Cin)).astype(np.float16)
    bias = (0.5 * r.standard_normal(Cout)).astype(np.float16)
    got = run_both_poisons(x, w, bias, None, act, stride, "dense")
    arena = Arena(CAPACITY, 0x55)
    xd, wd = arena.place(torch.from_numpy(x), 16, "x"), arena.place(torch.from_numpy(w), 16, "weight")
    bd = arena.place(torch.from_numpy(bias), 2, "bias")
    Ho, Wo = X.conv_out_hw(H, W, k, stride)
    out = arena.empty((B, Ho, Wo, Cout), torch.float16, 16, "out")
    assert h.bevops_conv_tile_f16(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, out.data_ptr(), B, H, W, Cin, Cout,
                                  k, stride, act, st) == L.SUCCESS
    arena.check()
    assert np.array_equal(out.cpu().numpy().view(np.int16), got)


# ---------------------------------------------------------------------------------------------- the Python side
def test_wrapper_equals_c_call_pads_channels_and_never_packs_under_capture():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.functions import yolox_ops as Y
    case = (1, 9, 14, 96, 96, 3, 1, "slice")
    x, w, bias, res, _ = lattice_case(case)
    want = run_both_poisons(x, w, bias, res, RELU, 1, "slice")
    wt = torch.from_numpy(w.copy()).cuda().permute(0, 3, 1, 2).contiguous()          # [Cout, Cin, k, k]
    buf = Y.nhwc_empty(1, 96 + 40, 9, 14, "cuda")
    buf.fill_(float("nan"))
    xs = buf[:, 8:104]
    xs.copy_(torch.from_numpy(x.copy()).cuda().permute(0, 3, 1, 2))
    rs = torch.from_numpy(res.copy()).cuda().permute(0, 3, 1, 2)
    dst = Y.nhwc_empty(1, 96 + 24, 9, 14, "cuda")
    dst.fill_(float("nan"))
    y = bev.conv_slice_nhwc(xs, wt, torch.from_numpy(bias.copy()).cuda(), "relu", rs, 1, out=dst[:, 16:112])
    assert y.data_ptr() == dst[:, 16:112].data_ptr()
    assert np.array_equal(y.permute(0, 2, 3, 1).cpu().numpy().view(np.int16), want)
    assert torch.isnan(dst[:, :16]).all() and torch.isnan(dst[:, 112:]).all()
    # an 80-channel layer on 96-channel tensors: zero rows and columns, exact zeros in the pad channels under SiLU
    w80 = wt[:80, :80].contiguous()
    x80 = xs.clone()
    x80[:, 80:] = 0
    y96 = bev.conv_slice_nhwc(x80, w80, None, "silu", out=Y.nhwc_empty(1, 96, 9, 14, "cuda"))
    assert torch.count_nonzero(y96[:, 80:]) == 0 and torch.count_nonzero(y96[:, :80]) > 0
    with pytest.raises(ValueError, match="16-byte"):
        bev.conv_slice_nhwc(buf[:, 4:100], wt)
    # a changed weight is repacked; never inside a capture
    p0 = Y.conv_slice_packed_weight(w80, 96, 96, build=False)
    assert p0 is not None
    w80.mul_(2.0)
    assert Y.conv_slice_packed_weight(w80, 96, 96, build=False) is None
    scratch = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="capturing"):
            bev.conv_slice_nhwc(x80, w80, None, "none", out=y96)
    del graph
    y2 = bev.conv_slice_nhwc(x80, w80, None, "none")
    y1 = bev.conv_slice_nhwc(x80, wt[:80, :80].contiguous(), None, "none")
    assert torch.equal(y2[:, :80], 2.0 * y1[:, :80])
