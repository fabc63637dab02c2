"""bevops_deconv4x4s2_s8 (csrc/deconv_s8.hip) through the C ABI in the guarded arena of tests/util_arena.py, under both
poisons.

* tolerance 0: int8 operands, power-of-two scales (scale_a 2^-5; per-channel weight scales 2^-9 .. 2^-2 with amplitudes
  127 .. 1 along the weight's dimension 1, or one scale 2^-9), bias integers * 2^-4, |sum| <= 2^24 (weight amplitudes
  <= 64 at Cin = 512: 2048 * 127 * 64 < 2^24): every product and sum of the epilogue is an fp32 number (asserted on the
  statement), so the result does not depend on what gets contracted; every output byte (fp16 bit) EQUALS the int64 /
  float64 statement.  scale_out = 2^floor(log2(std(v) / 48)) from the statement: outputs on both sides of the clamp, and
  exact ties (rne, not half-away).  Shapes: tests/util_deconv_s8.py SHAPES, each with and without bias, ReLU and
  per-channel scales, int8 and fp16 out.
* one-hot inputs whose every output names its tap; general scales inside the derived interval of
  tests/util_deconv_s8.py (exact outside the near-tie interval, whose share tests/test_deconv_s8_cpu.py bounds);
  non-finite containment; the Python wrapper, its packed-weight cache and the capture guard."""
import numpy as np
import pytest
import torch

import util_conv_slice_s8 as S
import util_deconv_s8 as D
import util_exact_dense as X
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 16 << 20


def _lib():
    from bevformer_tensorrt_amd.utils import lib as L
    return L, L.load_library(), L.current_stream_ptr(torch.device("cuda"))


def c_call(arena, x, w, ws, bias, relu, out, scale_a=D.S_A, scale_w=1.0, scale_out=1.0):
    """One call with every operand carved from `arena`; the weight through the Python pack -> [B, 2H, 2W, Cout] host array."""
    L, h, st = _lib()
    B, H, W, Cin = x.shape
    Cout = w.shape[1]
    xd = arena.place(torch.from_numpy(np.array(x)), 16, "x")
    wd = arena.place(torch.from_numpy(D.pack(w)), 16, "packed weight")
    wsd = None if ws is None else arena.place(torch.from_numpy(np.array(ws, dtype=np.float32)), 4, "w_scales")
    bd = None if bias is None else arena.place(torch.from_numpy(np.array(bias, dtype=np.float32)), 4, "bias")
    od = arena.empty((B, 2 * H, 2 * W, Cout), torch.int8 if out == "int8" else torch.float16, 16, "out")
    rc = h.bevops_deconv4x4s2_s8(xd.data_ptr(), scale_a, wd.data_ptr(), None if wsd is None else wsd.data_ptr(), scale_w,
                                 None if bd is None else bd.data_ptr(), L.I8 if out == "int8" else L.F16, od.data_ptr(),
                                 scale_out, B, H, W, Cin, Cout, int(relu), st)
    assert rc == L.SUCCESS
    arena.check()
    return od.cpu().numpy()


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
@pytest.mark.parametrize("out", ["int8", "fp16"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("per_channel", [False, True], ids=["tensor", "channel"])
@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_lattice_bits(shape, per_channel, with_bias, relu, out):
    x, w, ws, scale_w, bias, acc = D.lattice_case(shape, out, per_channel)
    want, s_out, t = D.lattice_statement(shape, out, per_channel, with_bias, relu)
    # the order-of-operations statement agrees with the lattice statement
    _assert_equal(D.exact_output(acc, D.S_A, scale_w, ws, bias if with_bias else None, int(relu), None, 1.0, s_out, out), want)
    if t is not None and want.size >= 1000:
        ties, beyond = X.int8_shares(t)
        print(f"scale_out 2^{int(np.log2(s_out))}: {ties:.3%} exact ties, {beyond:.3%} beyond +-127")
        assert ties > 0 and beyond > 0 and (want == 127).any() and ((want == -127).any() or relu)
    got = run_both_poisons(x, w, ws, bias if with_bias else None, relu, out, scale_w=scale_w, scale_out=s_out)
    _assert_equal(got, want)
    assert want.any()


# ---------------------------------------------------------------------------------------------- which tap lands where
@pytest.mark.parametrize("b0,y0,x0", [(1, 0, 0), (1, 4, 5), (1, 0, 3), (1, 2, 0), (1, 2, 3), (0, 4, 5)],
                         ids=["corner", "far-corner", "edge-top", "edge-left", "interior", "last-pixel-of-image-0"])
@pytest.mark.parametrize("out", ["int8", "fp16"])
def test_one_hot_names_its_tap(b0, y0, x0, out):
    """x = 1 at one pixel and channel, w[ci, co, ky, kx] = 1 + 4 ky + kx: output pixel (oy, ox) must hold the number of
    tap (ky, kx) = (oy - 2 y0 + 1, ox - 2 x0 + 1) when that is a tap, and zero otherwise -- in the other image too (the
    last pixel of image 0 is followed in memory by the first of image 1)."""
    B, H, W, Cin, Cout, c0 = 2, 5, 6, 128, 16, 77
    x = np.zeros((B, H, W, Cin), np.int8)
    x[b0, y0, x0, c0] = 1
    taps = (1 + 4 * np.arange(4)[:, None] + np.arange(4)[None, :]).astype(np.int8)
    w = np.ascontiguousarray(np.broadcast_to(taps, (Cin, Cout, 4, 4)))
    want = np.zeros((B, 2 * H, 2 * W, Cout), np.int64)
    for oy in range(2 * H):
        for ox in range(2 * W):
            ky, kx = oy - 2 * y0 + 1, ox - 2 * x0 + 1
            if 0 <= ky < 4 and 0 <= kx < 4:
                want[b0, oy, ox, :] = taps[ky, kx]
    assert np.array_equal(want, D.sums(x, w))                    # (the statement above is conv_transpose2d)
    got = run_both_poisons(x, w, None, None, False, out, scale_a=1.0, scale_out=1.0)
    assert np.array_equal(got.astype(np.int64), want), np.argwhere(got.astype(np.int64) != want)[:8]


# ---------------------------------------------------------------------------------------------- general scales
@pytest.mark.parametrize("out", ["int8", "fp16"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("case", D.GENERAL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_general_scales_within_the_derived_interval(case, relu, out):
    """Non-power-of-two scales: every output within one step of the float64 statement and EQUAL to it wherever the
    statement is farther than the derived delta from a rounding boundary (lo == hi there)."""
    x, w, ws, bias, acc, scale_a = D.general_case(case)
    scale_out, t, delta, lo, hi, y_lo, y_hi = D.general_statement(case, relu)
    got = run_both_poisons(x, w, ws, bias, relu, out, scale_a=float(scale_a), scale_out=float(scale_out))
    if out == "int8":
        share = S.check_interval(got, lo, hi)
        off = float((got != np.clip(np.rint(t), -127, 127)).mean())
        print(f"delta max {delta.max():.2e} steps; {share:.4%} within delta of a half-integer; {off:.4%} differ from rne(t)")
    else:
        lo16, hi16 = y_lo.astype(np.float16), y_hi.astype(np.float16)
        assert ((got >= lo16) & (got <= hi16)).all()
        assert float((lo16 != hi16).mean()) < 0.01


# ---------------------------------------------------------------------------------------------- non-finite containment
@pytest.mark.parametrize("out", ["int8", "fp16"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_non_finite_bias_stays_in_its_channel(relu, out):
    """A NaN / +inf / -inf bias touches only its own output channel.  int8: NaN -> -127 (max(NaN, -127) = -127; with ReLU
    max(NaN, 0) = 0 first), +inf -> 127, -inf -> -127 (0 with ReLU); fp16: the value goes through as it is."""
    case = (1, 9, 14, 128, 64)
    x, w, ws, bias, acc, scale_a = D.general_case(case)
    args = dict(scale_a=float(scale_a), scale_out=0.11)
    clean = c_call(Arena(CAPACITY, POISONS[0]), x, w, ws, bias, relu, out, **args)
    bad = bias.copy()
    bad[5], bad[17], bad[40] = np.nan, np.inf, -np.inf
    got = c_call(Arena(CAPACITY, POISONS[0]), x, w, ws, bad, relu, out, **args)
    others = np.ones(64, bool)
    others[[5, 17, 40]] = False
    assert np.array_equal(_bits(got[..., others]), _bits(clean[..., others]))
    if out == "int8":
        assert (got[..., 5] == (0 if relu else -127)).all() and (got[..., 17] == 127).all()
        assert (got[..., 40] == (0 if relu else -127)).all()
    else:
        assert (got[..., 5] == 0).all() if relu else np.isnan(got[..., 5]).all()
        assert np.isposinf(got[..., 17]).all()
        assert (got[..., 40] == 0).all() if relu else np.isneginf(got[..., 40]).all()


# ---------------------------------------------------------------------------------------------- the Python side
def test_wrapper_equals_c_call_caches_the_pack_and_never_packs_under_capture():
    from bevformer_tensorrt_amd.functions import deconv as DC
    from bevformer_tensorrt_amd.utils import lib as L
    shape = D.SHAPES[2]
    for out, dt in (("int8", torch.int8), ("fp16", torch.float16)):
        x, w, ws, scale_w, bias, acc = D.lattice_case(shape, out, True)
        want, s_out, _ = D.lattice_statement(shape, out, True, True, True)
        xd = torch.from_numpy(x.copy()).cuda().permute(0, 3, 1, 2)
        wd, wsd, bd = (torch.from_numpy(a.copy()).cuda() for a in (w, ws, bias))
        y = DC.conv_transpose2d_q_nhwc(xd, D.S_A, wd, wsd, bd, True, s_out if out == "int8" else None, dt)
        assert y.is_contiguous(memory_format=torch.channels_last) and y.dtype == dt
        _assert_equal(y.permute(0, 2, 3, 1).cpu().numpy(), want)
        p0 = DC.deconv_packed_weight(wd, build=False)
        assert p0 is not None and p0.dtype == torch.int8 and torch.equal(p0.cpu(), torch.from_numpy(D.pack(w)))
        assert DC.conv_transpose2d_q_nhwc(xd[:0], D.S_A, wd, wsd, bd, True, 1.0, dt).shape == (0, w.shape[1], 24, 22)
        wd.neg_()                                                         # a changed weight: the cached pack is stale
        assert DC.deconv_packed_weight(wd, build=False) is None
        scratch = torch.zeros(8, device="cuda")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            scratch.add_(1.0)                                             # (the capture holds one node of its own)
            with pytest.raises(RuntimeError, match="capturing"):
                DC.conv_transpose2d_q_nhwc(xd, D.S_A, wd, wsd, bd, True, 1.0, dt)
        del graph
        assert DC.deconv_packed_weight(wd, build=False) is None
    xd = torch.zeros(1, 32, 2, 2, dtype=torch.int8, device="cuda").contiguous(memory_format=torch.channels_last)
    with pytest.raises(L.BevopsError) as e:
        DC.conv_transpose2d_q_nhwc(xd, 1.0, torch.zeros(32, 16, 4, 4, dtype=torch.int8, device="cuda"), None, None, False, 1.0)
    assert e.value.status == L.NOT_SUPPORTED
