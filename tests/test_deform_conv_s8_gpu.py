"""bevops_deform_conv3x3_nhwc_s8 (csrc/deform_conv_s8.hip) through the C ABI in the guarded arena of tests/util_arena.py,
under both poisons, every byte of the output buffer outside the output slice compared; the statements are those of
tests/util_deform_conv_s8.py (their premises: tests/test_deform_conv_s8_cpu.py).

Channel shapes (Cin / g, Cout / g, g): (32, 32, 1), (64, 64, 4), (96, 32, 2), (32, 96, 2), (64, 96, 1), (96, 96, 4) --
96 covers the 32-byte k-chunk and the half-empty second channel tile.  Pixels: (1, 1, 1), one pixel with every tap partly
outside, and (2, 9, 15): 270 pixels, tiles cross the image boundary, the tail has 14 rows.  Pitches: 'dense'
(pitch == channels) and 'slice' (x and out inside wider buffers).

* exact bytes on the offset lattice with power-of-two scales, int8 and fp16 out (tolerance 0: the blend, the sums and
  the epilogue are exact); ties and both saturations occur (asserted on the 270-pixel cases);
* one-hot weights: the output byte IS the column byte, on the lattice (equal) and on Gaussian fp16 offsets (equal to
  rne(s64) except within EPS = 4 * 2^-24 * 127 of a half-integer, where either neighbour passes);
* general scales on the lattice inside the epilogue's derived interval;
* equality with bevops_conv_slice_s8 at zero offsets and at offsets (0, +1); junk behind channel 18; non-finite and huge
  offsets; replay under a captured graph; the wrapper with out= slices and its errors."""
import numpy as np
import pytest
import torch

import util_conv_slice_s8 as S
import util_deform_conv_s8 as D
import util_exact_dense as X
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 8 << 20
BIG = D.PIXELS[1]


def _lib():
    from bevformer_tensorrt_amd.utils import lib as L
    return L, L.load_library(), L.current_stream_ptr(torch.device("cuda"))


def _place_slice(arena, values, pitch, c0, name):
    B, H, W, C = values.shape
    t = torch.from_numpy(np.array(values))
    buf = arena.empty((B, H, W, pitch), t.dtype, 16, name)
    view = buf[..., c0:c0 + C]
    view.copy_(t)
    return buf, view


def c_call(arena, x, off, w, ws, bias, groups, layout, out, relu=0, scale_a=D.S_A, scale_w=1.0, scale_out=1.0):
    """One call with every operand carved from `arena` -> the output slice [B, H, W, Cout] (int8 or fp16 host array)."""
    L, h, st = _lib()
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    odt = torch.int8 if out == "int8" else torch.float16
    wd = arena.place(torch.from_numpy(np.array(w)), 16, "weight")
    wsd = None if ws is None else arena.place(torch.from_numpy(np.array(ws, dtype=np.float32)), 16, "w_scales")
    bd = None if bias is None else arena.place(torch.from_numpy(np.array(bias, dtype=np.float32)), 16, "bias")
    od = arena.place(torch.from_numpy(np.array(off)), 16, "offset")
    xp, xc0 = (Cin, 0) if layout == "dense" else (Cin + 48, 16)
    op, oc0 = (Cout, 0) if layout == "dense" else ((Cout + 32, 16) if out == "int8" else (Cout + 24, 8))
    _, xv = _place_slice(arena, x, xp, xc0, "x")
    obuf = arena.empty((B, H, W, op), odt, 16, "out")
    ov = obuf[..., oc0:oc0 + Cout]
    before = obuf.cpu().numpy().view(np.uint8).copy()
    rc = h.bevops_deform_conv3x3_nhwc_s8(xv.data_ptr(), xp, scale_a, od.data_ptr(), off.shape[-1], wd.data_ptr(),
                                         None if wsd is None else wsd.data_ptr(), scale_w,
                                         None if bd is None else bd.data_ptr(), L.I8 if out == "int8" else L.F16,
                                         ov.data_ptr(), op, scale_out, relu, B, H, W, Cin, Cout, groups, st)
    assert rc == L.SUCCESS
    arena.check()
    after = obuf.cpu().numpy()
    mask = np.zeros(after.shape, bool)
    mask[..., oc0:oc0 + Cout] = True
    mask8 = np.repeat(mask, after.itemsize, axis=-1)
    assert np.array_equal(after.view(np.uint8)[~mask8], before[~mask8]), "bytes of the output buffer outside the slice were written"
    return after[..., oc0:oc0 + Cout].copy()


def run_both_poisons(*args, **kw):
    got = [c_call(Arena(CAPACITY, poison), *args, **kw) for poison in POISONS]
    assert np.array_equal(got[0].view(np.uint8), got[1].view(np.uint8)), "results differ between the two poisons"
    return got[0]


def _bits(a):
    return a.view(np.int16) if a.dtype == np.float16 else a


def _assert_equal(got, want):
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (f"{len(bad)} of {want.size} outputs differ, first at {tuple(bad[0])}: got "
                           f"{got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


# ---------------------------------------------------------------------------------------------- tolerance 0
@pytest.mark.parametrize("layout,out", [("dense", "int8"), ("slice", "int8"), ("slice", "fp16"), ("dense", "fp16")])
@pytest.mark.parametrize("px", D.PIXELS, ids=lambda p: "x".join(map(str, p)))
@pytest.mark.parametrize("ch", D.CHANNELS, ids=lambda c: "x".join(map(str, c)))
def test_lattice_bits(ch, px, layout, out):
    x, off, w, ws, bias, s64, acc = D.lattice_case(ch, px)
    for full, relu in ((True, 0), (False, 1)):
        want, s_out, t = D.lattice_statement(ch, px, full, relu, out)
        if t is not None and px == BIG:
            ties, beyond = X.int8_shares(t)
            print(f"scale_out 2^{int(np.log2(s_out))}: {ties:.3%} exact ties, {beyond:.3%} beyond +-127")
            assert ties > 0 and beyond > 0 and (want == 127).any() and ((want == -127).any() or relu)
        got = run_both_poisons(x, off, w, ws, bias if full else None, ch[2], layout, out, relu=relu, scale_out=s_out)
        _assert_equal(got, want)
        assert want.any() or px != BIG


# ---------------------------------------------------------------------------------------------- one-hot weights
def _picked(s64, picks, ch):
    cin_g, cout_g, _ = ch
    return np.stack([s64[..., t, (co // cout_g) * cin_g + ci] for co, (t, ci) in enumerate(picks)], axis=-1)


@pytest.mark.parametrize("px", D.PIXELS, ids=lambda p: "x".join(map(str, p)))
@pytest.mark.parametrize("ch", D.CHANNELS, ids=lambda c: "x".join(map(str, c)))
def test_one_hot_weights_show_the_column_on_the_lattice(ch, px):
    """One tap, one channel, unit scales: the output byte IS the column byte -- every (tap, channel) localised."""
    x, off, _, _, _, s64, _ = D.lattice_case(ch, px)
    w, picks = D.one_hot_weights(X._rng("deform_conv_s8.onehot", ch), ch)
    want = D.column(_picked(s64, picks, ch))
    got = run_both_poisons(x, off, w, None, None, ch[2], "slice", "int8", scale_a=1.0, scale_out=1.0)
    _assert_equal(got, want)
    if px == BIG:
        sel = _picked(s64, picks, ch)
        assert (np.abs(sel - np.floor(sel) - 0.5) == 0).any() and (want != 0).mean() > 0.5


@pytest.mark.parametrize("seed", D.GENERAL_SEEDS)
@pytest.mark.parametrize("ch", D.CHANNELS, ids=lambda c: "x".join(map(str, c)))
def test_one_hot_weights_on_general_offsets(ch, seed):
    x, off, w, picks, sel = D.general_case(ch, seed)
    lo, hi = D.column_interval(sel)
    got = run_both_poisons(x, off, w, None, None, ch[2], "dense", "int8", scale_a=1.0, scale_out=1.0)
    excused = float((lo != hi).mean())
    print(f"{ch} seed {seed}: {excused:.2e} of {sel.size} excused, {float((got != D.column(sel)).mean()):.2e} on the other neighbour")
    assert excused <= D.NEAR_TIE_CAP
    S.check_interval(got, lo, hi, cap=D.NEAR_TIE_CAP)


# ---------------------------------------------------------------------------------------------- general scales
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("ch", D.CHANNELS, ids=lambda c: "x".join(map(str, c)))
def test_general_scales_within_the_derived_interval(ch, relu):
    x, off, w, _, _, _, acc = D.lattice_case(ch, BIG)
    ws, bias, s_out = D.general_scale_operands(ch)
    _, _, lo, hi = D.linear_interval(acc, D.GENERAL_S_A, 1.0, ws, bias, relu, s_out)
    got = run_both_poisons(x, off, w, ws, bias, ch[2], "slice", "int8", relu=relu, scale_a=D.GENERAL_S_A, scale_out=s_out)
    share = S.check_interval(got, lo, hi)
    want = S.exact_output(acc, D.GENERAL_S_A, 1.0, ws, bias, relu, None, 1.0, s_out, "int8")
    print(f"{ch} relu {relu}: {share:.2e} excused, {float((got != want).mean()):.2e} differ from the fp32 statement")
    # fp16 out: one rounding of the fp32 value -- the extended-precision statement of the same operations
    got16 = run_both_poisons(x, off, w, ws, bias, ch[2], "dense", "fp16", relu=relu, scale_a=D.GENERAL_S_A)
    _assert_equal(got16, S.exact_output(acc, D.GENERAL_S_A, 1.0, ws, bias, relu, None, 1.0, 1.0, "fp16"))


# ---------------------------------------------------------------------------------------------- an independent kernel
def _conv_slice(arena, x, w, ws, bias, out, scale_out):
    L, h, st = _lib()
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    xd = arena.place(torch.from_numpy(np.array(x)), 16, "x")
    wd = arena.place(torch.from_numpy(np.array(w)), 16, "weight")
    wsd = arena.place(torch.from_numpy(np.array(ws, dtype=np.float32)), 16, "w_scales")
    bd = arena.place(torch.from_numpy(np.array(bias, dtype=np.float32)), 16, "bias")
    od = arena.empty((B, H, W, Cout), torch.int8 if out == "int8" else torch.float16, 16, "out")
    rc = h.bevops_conv_slice_s8(xd.data_ptr(), Cin, D.S_A, wd.data_ptr(), wsd.data_ptr(), 1.0, bd.data_ptr(), None, 0, 1.0,
                                L.I8 if out == "int8" else L.F16, od.data_ptr(), Cout, scale_out, B, H, W, Cin, Cout, 3, 1,
                                0, st)
    assert rc == L.SUCCESS
    arena.check()
    return od.cpu().numpy()


@pytest.mark.parametrize("out", ["int8", "fp16"])
@pytest.mark.parametrize("ch", [(32, 32, 1), (64, 96, 1)], ids=lambda c: "x".join(map(str, c)))
def test_equals_conv_slice_s8_at_zero_and_unit_offsets(ch, out):
    """groups = 1.  Zero offsets: the plain 3 x 3 convolution.  All offsets (0, +1): that convolution on the input shifted
    by one column -- with the input's column 0 zero, because the plain convolution pads the SHIFTED image on its left
    where the deformable one reads column 0 of the un-shifted one."""
    x, _, w, ws, bias, _, _ = D.lattice_case(ch, BIG)
    x = np.array(x)
    x[:, :, 0] = 0
    B, H, W, _ = x.shape
    _, s_out, _ = D.lattice_statement(ch, BIG, True, 0, "int8")
    zero = np.zeros((B, H, W, 18), np.float16)
    got = run_both_poisons(x, zero, w, ws, bias, 1, "dense", out, scale_out=s_out)
    _assert_equal(got, _conv_slice(Arena(CAPACITY, POISONS[0]), x, w, ws, bias, out, s_out))
    unit = zero.copy()
    unit[..., 1::2] = 1.0
    shifted = np.zeros_like(x)
    shifted[:, :, :-1] = x[:, :, 1:]
    got = run_both_poisons(x, unit, w, ws, bias, 1, "dense", out, scale_out=s_out)
    want = _conv_slice(Arena(CAPACITY, POISONS[0]), shifted, w, ws, bias, out, s_out)
    _assert_equal(got, want)
    assert want.any()


# ---------------------------------------------------------------------------------------------- the offset rows
def test_channels_behind_18_are_never_read():
    ch = (64, 64, 4)
    x, off, w, ws, bias, _, _ = D.lattice_case(ch, BIG)
    want, s_out, _ = D.lattice_statement(ch, BIG, True, 0, "int8")
    r = X._rng("deform_conv_s8.junk")
    for oc in (24, 32):
        wide = np.empty(off.shape[:3] + (oc,), np.float16)
        wide[..., :18] = off
        junk = r.normal(0.0, 30.0, size=off.shape[:3] + (oc - 18,)).astype(np.float16)          # mask-like logits ...
        junk[r.random(junk.shape) < 0.2] = np.float16("nan")                                      # ... and worse
        junk[r.random(junk.shape) < 0.1] = np.float16("inf")
        wide[..., 18:] = junk
        _assert_equal(run_both_poisons(x, wide, w, ws, bias, ch[2], "slice", "int8", scale_out=s_out), want)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf"), 60000.0], ids=str)
def test_non_finite_and_huge_offsets_stay_in_their_pixel(bad):
    ch = (96, 32, 2)
    x, off, w, ws, bias, _, _ = D.lattice_case(ch, BIG)
    base, s_out, _ = D.lattice_statement(ch, BIG, True, 0, "int8")
    b, y, xx = 1, 8, 14                                                       # the last pixel: in the 14-row tail tile
    o = np.array(off)
    o[b, y, xx, 0:18:4] = bad
    o[b, y, xx, 3:18:4] = bad
    want = S.exact_output(D.sums(D.column(D.column_s64(x, o)), w, ch[2]), D.S_A, 1.0, ws, bias, 0, None, 1.0, s_out, "int8")
    got = run_both_poisons(x, o, w, ws, bias, ch[2], "slice", "int8", scale_out=s_out)
    _assert_equal(got, want)
    keep = np.ones(base.shape[:3], bool)
    keep[b, y, xx] = False
    assert np.array_equal(got[keep], base[keep]) and not np.array_equal(got[b, y, xx], base[b, y, xx])


# ---------------------------------------------------------------------------------------------- the wrapper
def _device_case(ch, px=BIG):
    x, off, w, ws, bias, _, acc = D.lattice_case(ch, px)
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    return t(x).permute(0, 3, 1, 2), t(off).permute(0, 3, 1, 2), t(w), t(ws), t(bias)


def test_wrapper_with_out_slices_and_graph_replay():
    from bevformer_tensorrt_amd.functions import deform_conv2d_q_nhwc
    from bevformer_tensorrt_amd.functions.yolox_ops import nhwc_empty
    ch = (64, 64, 4)
    xq, off, w, ws, bias = _device_case(ch)
    want, s_out, _ = D.lattice_statement(ch, BIG, True, 0, "int8")
    want16, _, _ = D.lattice_statement(ch, BIG, True, 0, "fp16")
    B, C, H, W = xq.shape
    # x a slice of a wider buffer, out a slice of another
    xbuf = nhwc_empty(B, C + 64, H, W, xq.device, torch.int8)
    xbuf.fill_(77)
    xs = xbuf[:, 32:32 + C]
    xs.copy_(xq)
    obuf = nhwc_empty(B, C + 48, H, W, xq.device, torch.int8)
    obuf.fill_(-5)
    y = deform_conv2d_q_nhwc(xs, D.S_A, off, w, ws, bias, ch[2], out=obuf[:, 16:16 + C], scale_out=s_out)
    assert y.data_ptr() == obuf[:, 16:16 + C].data_ptr()
    _assert_equal(y.permute(0, 2, 3, 1).cpu().numpy(), want)
    assert bool((obuf[:, :16] == -5).all()) and bool((obuf[:, 16 + C:] == -5).all())
    # without out=, both dtypes; ReLU and no bias through the keyword
    eager = deform_conv2d_q_nhwc(xq, D.S_A, off, w, ws, bias, ch[2], scale_out=s_out)
    _assert_equal(eager.permute(0, 2, 3, 1).cpu().numpy(), want)
    assert eager.dtype == torch.int8 and eager.is_contiguous(memory_format=torch.channels_last)
    y16 = deform_conv2d_q_nhwc(xq, D.S_A, off, w, ws, bias, ch[2], out_dtype=torch.float16)
    _assert_equal(y16.permute(0, 2, 3, 1).cpu().numpy(), want16)
    wr, _, _ = D.lattice_statement(ch, BIG, False, 1, "fp16")
    yr = deform_conv2d_q_nhwc(xq, D.S_A, off, w, ws, None, ch[2], out_dtype=torch.float16, relu=True)
    _assert_equal(yr.permute(0, 2, 3, 1).cpu().numpy(), wr)
    # replay under a captured graph: bit-equal to the eager call
    static = torch.empty_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        deform_conv2d_q_nhwc(xq, D.S_A, off, w, ws, bias, ch[2], out=static, scale_out=s_out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        deform_conv2d_q_nhwc(xq, D.S_A, off, w, ws, bias, ch[2], out=static, scale_out=s_out)
    static.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)
    # an empty batch launches nothing
    e = deform_conv2d_q_nhwc(xq[:0], D.S_A, off[:0], w, ws, bias, ch[2], scale_out=s_out)
    assert tuple(e.shape) == (0, C, H, W)


def test_wrapper_errors():
    from bevformer_tensorrt_amd.functions import deform_conv2d_q_nhwc
    from bevformer_tensorrt_amd.utils.lib import NOT_SUPPORTED, BevopsError
    ch = (32, 32, 1)
    xq, off, w, ws, bias = _device_case(ch, D.PIXELS[0])
    ok = dict(scale_out=0.5)
    assert deform_conv2d_q_nhwc(xq, 1.0, off, w, ws, bias, 1, **ok).shape == xq.shape
    with pytest.raises(TypeError):
        deform_conv2d_q_nhwc(xq.half(), 1.0, off, w, ws, bias, 1, **ok)
    with pytest.raises(TypeError):
        deform_conv2d_q_nhwc(xq, 1.0, off.float(), w, ws, bias, 1, **ok)
    with pytest.raises(ValueError, match="w_q_taps"):
        deform_conv2d_q_nhwc(xq, 1.0, off, w.permute(0, 3, 1, 2), ws, bias, 1, **ok)
    with pytest.raises(ValueError, match="groups"):
        deform_conv2d_q_nhwc(xq, 1.0, off, w, ws, bias, 2, **ok)
    with pytest.raises(ValueError, match="cover"):
        deform_conv2d_q_nhwc(xq, 1.0, off.expand(2, -1, -1, -1).contiguous(memory_format=torch.channels_last), w, ws, bias, 1, **ok)
    with pytest.raises(ValueError, match="18"):
        deform_conv2d_q_nhwc(xq, 1.0, off[:, :16].contiguous(memory_format=torch.channels_last), w, ws, bias, 1, **ok)
    with pytest.raises(ValueError, match="scale"):
        deform_conv2d_q_nhwc(xq, 0.0, off, w, ws, bias, 1, **ok)
    with pytest.raises(ValueError, match="scale"):
        deform_conv2d_q_nhwc(xq, 1.0, off, w, ws, bias, 1, scale_out=float("inf"))
    with pytest.raises((ValueError, TypeError)):
        deform_conv2d_q_nhwc(xq, 1.0, off, w, ws, bias, 1)                    # int8 out needs scale_out
    with pytest.raises(ValueError, match="w_scales"):
        deform_conv2d_q_nhwc(xq, 1.0, off, w, ws[:16], bias, 1, **ok)
    with pytest.raises(ValueError, match="bias"):
        deform_conv2d_q_nhwc(xq, 1.0, off, w, ws, bias.double(), 1, **ok)
    with pytest.raises(ValueError, match="out_dtype"):
        deform_conv2d_q_nhwc(xq, 1.0, off, w, ws, bias, 1, out_dtype=torch.float32, **ok)
    with pytest.raises(ValueError, match="out is"):
        deform_conv2d_q_nhwc(xq, 1.0, off, w, ws, bias, 1, out=torch.empty_like(xq, dtype=torch.float16), **ok)
    with pytest.raises(ValueError, match="out must be"):
        deform_conv2d_q_nhwc(xq, 1.0, off, w, ws, bias, 1, out=torch.empty_like(xq)[:, :16], **ok)
    with pytest.raises(BevopsError) as e:                                     # 16 channels per group
        deform_conv2d_q_nhwc(xq, 1.0, off, w[:, :, :, :16].contiguous(), ws, bias, 2, **ok)
    assert e.value.status == NOT_SUPPORTED
