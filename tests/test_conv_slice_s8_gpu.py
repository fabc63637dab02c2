"""bevops_conv_slice_s8 (csrc/conv_slice_s8.hip) through the C ABI in the guarded arena of tests/util_arena.py, under both
poisons, every byte of the output buffer outside the output slice compared.

Shapes: B in {1, 2}; maps 7 x 9 (63 rows) and 12 x 11 (132 rows: across a row-tile edge), odd sizes with stride 2; Cin in
{32, 64, 96, 160} with k in {1, 3}: K = 32 (half a step), 160 (2.5), 288 (4.5, steps that straddle taps), 864 (13.5),
1440 (22.5); Cout in {16, 48, 64, 144} (both tile widths, a column-tile edge) and 88 with fp16 out.  Layouts: 'dense'
(pitch == channels), 'slice' (x, identity and out are slices of wider buffers), 'same' (x and out are slices of ONE
buffer), 'inplace' (out IS the identity's slice).

* exact (act none / ReLU): int8 operands, power-of-two scales (scale_a 2^-5, per-channel weight scales 2^-9 .. 2^-2 with
  amplitudes 127 .. 1, scale_res 2^-5, scale_out a power of two), bias integers * 2^-4: every product and sum of the
  epilogue is an fp32 number (asserted on the statement), so the result does not depend on what gets contracted;
  every output byte (fp16 bit) EQUALS the int64 / float64 statement.  scale_out = 2^floor(log2(std(v) / 48)) from the
  statement: outputs on both sides of the clamp, and exact ties (rne, not half-away).
* one-hot taps, tail isolation, SiLU with general scales inside the derived interval of tests/util_conv_slice_s8.py,
  equality with bevops_conv_tile_int8, non-finite containment, the int32 bound."""
import functools

import numpy as np
import pytest
import torch

import util_conv_slice_s8 as S
import util_exact_dense as X
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 16 << 20
NONE, RELU, SILU = 0, 1, 2
S_A, S_RES = 2.0 ** -5, 2.0 ** -5


def _lib():
    from bevformer_tensorrt_amd.utils import lib as L
    return L, L.load_library(), L.current_stream_ptr(torch.device("cuda"))


def _place_slice(arena, values, pitch, c0, name, align=16):
    """values [B, H, W, C] as channels c0 .. c0 + C of a poisoned [B, H, W, pitch] buffer -> (buffer, slice view)."""
    B, H, W, C = values.shape
    t = torch.from_numpy(np.array(values))
    buf = arena.empty((B, H, W, pitch), t.dtype, align, name)
    view = buf[..., c0:c0 + C]
    view.copy_(t)
    return buf, view


def c_call(arena, x, w, ws, bias, res, act, stride, layout, out, scale_a=S_A, scale_w=1.0, scale_res=S_RES, scale_out=1.0):
    """One call with every operand carved from `arena` -> the output slice [B, Ho, Wo, Cout] (int8 or fp16 host array)."""
    L, h, st = _lib()
    B, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    Ho, Wo = X.conv_out_hw(H, W, k, stride)
    odt = torch.int8 if out == "int8" else torch.float16
    wd = arena.place(torch.from_numpy(np.array(w)), 16, "weight")
    wsd = None if ws is None else arena.place(torch.from_numpy(np.array(ws, dtype=np.float32)), 4, "w_scales")
    bd = None if bias is None else arena.place(torch.from_numpy(np.array(bias, dtype=np.float32)), 4, "bias")
    rv, rp = None, 0
    if layout == "same":
        assert stride == 1 and out == "int8"
        pitch = Cin + Cout + 16
        buf, xv = _place_slice(arena, x, pitch, 0, "x|out")
        obuf, oc0, op, xp = buf, Cin, pitch, pitch
    else:
        xp, xc0 = (Cin, 0) if layout == "dense" else (Cin + 48, 16)
        op, oc0 = (Cout, 0) if layout == "dense" else ((Cout + 32, 16) if out == "int8" else (Cout + 24, 8))
        _, xv = _place_slice(arena, x, xp, xc0, "x")
        if layout == "inplace":
            assert out == "int8" and res is not None
            obuf, _ = _place_slice(arena, res, op, oc0, "identity|out")
        else:
            obuf = arena.empty((B, Ho, Wo, op), odt, 16, "out")
    ov = obuf[..., oc0:oc0 + Cout]
    if res is not None:
        if layout == "inplace":
            rv, rp = ov, op
        else:
            # (an int8 identity's pitch is a multiple of 16: behind 88 fp16 output channels it cannot be the channel count)
            rp = (Cout if layout == "dense" else Cout + 16) + 15 & ~15
            _, rv = _place_slice(arena, res, rp, 0, "identity")
    before = obuf.cpu().numpy().view(np.uint8).copy()
    rc = h.bevops_conv_slice_s8(xv.data_ptr(), xp, scale_a, wd.data_ptr(), None if wsd is None else wsd.data_ptr(), scale_w,
                                None if bd is None else bd.data_ptr(), None if rv is None else rv.data_ptr(), rp, scale_res,
                                L.I8 if out == "int8" else L.F16, ov.data_ptr(), op, scale_out, B, H, W, Cin, Cout, k,
                                stride, act, st)
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
# (B, H, W, Cin, Cout, ksize, stride, layout, out)
CASES = ((1, 7, 9, 32, 16, 3, 1, "slice", "int8"), (2, 7, 9, 96, 48, 3, 2, "slice", "int8"),
         (1, 12, 11, 160, 64, 1, 1, "dense", "int8"), (2, 12, 11, 64, 144, 3, 1, "same", "int8"),
         (1, 12, 11, 96, 144, 1, 2, "slice", "int8"), (2, 7, 9, 160, 88, 3, 1, "slice", "fp16"),
         (1, 12, 11, 32, 88, 1, 1, "dense", "fp16"), (2, 7, 9, 32, 64, 3, 2, "inplace", "int8"),
         (1, 7, 9, 64, 16, 1, 1, "dense", "int8"), (2, 12, 11, 96, 48, 3, 1, "same", "int8"))


@functools.lru_cache(maxsize=None)
def lattice_case(case):
    B, H, W, Cin, Cout, k, stride, _, _ = case
    r = X._rng("conv_slice_s8", case)
    x = X.gen_int8(r, (B, H, W, Cin))
    w, ws = X.gen_weights_int8(r, Cout, k * k * Cin, True)
    w = w.reshape(Cout, k, k, Cin)
    bias = X.gen_bias(r, Cout, "s8")
    Ho, Wo = X.conv_out_hw(H, W, k, stride)
    res = X.gen_identity(r, (B, Ho, Wo, Cout), "s8", "int8")
    acc = S.sums(x, w, k, stride)
    for a in (x, w, ws, bias, res, acc):
        a.setflags(write=False)
    return x, w, ws, bias, res, acc


def lattice_statement(case, full, act):
    """-> (want, scale_out, t): every step asserted to be an fp32 number, so no contraction can change it."""
    x, w, ws, bias, res, acc = lattice_case(case)
    out = case[8]
    v = X.f32_exact(X.f32_exact(acc.astype(np.float64), "(float)sum") * (S_A * ws.astype(np.float64)), "* scale")
    if full:
        v = X.f32_exact(v + bias.astype(np.float64), "+ bias")
    if act == RELU:
        v = np.maximum(v, 0.0)
    if full:
        v = X.f32_exact(v + res.astype(np.float64) * S_RES, "+ identity")        # the identity BEHIND the activation
    if out == "fp16":
        return v.astype(np.float32).astype(np.float16), 1.0, None
    s_out = 2.0 ** int(np.floor(np.log2(v.std() / 48.0)))
    t = X.f32_exact(v / s_out, "/ scale_out")
    return np.clip(np.rint(t), -127, 127).astype(np.int8), s_out, t


@pytest.mark.parametrize("act", [NONE, RELU], ids=["linear", "relu"])
@pytest.mark.parametrize("epi", ["plain", "bias+identity"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_lattice_bits(case, epi, act):
    x, w, ws, bias, res, acc = lattice_case(case)
    full = epi != "plain"
    layout, out = case[7], case[8]
    if layout == "inplace" and not full:
        layout = "slice"                         # (out identical to the identity needs an identity)
    want, s_out, t = lattice_statement(case, full, act)
    # the order-of-operations statement of tests/util_conv_slice_s8.py agrees with the lattice statement
    _assert_equal(S.exact_output(acc, S_A, 1.0, ws, bias if full else None, act, res if full else None, S_RES, s_out, out), want)
    if t is not None:
        ties, beyond = X.int8_shares(t)
        print(f"scale_out 2^{int(np.log2(s_out))}: {ties:.3%} exact ties, {beyond:.3%} beyond +-127")
        assert ties > 0 and beyond > 0 and (want == 127).any() and ((want == -127).any() or act == RELU)
    got = run_both_poisons(x, w, ws, bias if full else None, res if full else None, act, case[6], layout, out, scale_out=s_out)
    _assert_equal(got, want)
    assert want.any()


# ---------------------------------------------------------------------------------------------- one-hot taps
@pytest.mark.parametrize("cin,k,stride", [(32, 3, 1), (96, 3, 1), (96, 3, 2), (160, 1, 1), (160, 3, 1), (64, 3, 2)])
def test_one_hot_tap_localisation(cin, k, stride):
    """ONE non-zero pixel (every channel c holds 1 + c % 100) and ONE non-zero weight per output channel, each at its
    own (ky, kx, ci): 48 positions spread over K, the first and last chunk of every tap and the tail chunk among them.
    Output channel co is non-zero at exactly the one pixel the statement names (none when the tap reads outside the
    map or between the strides): a wrong tap delta or k-chunk map moves or loses it."""
    B, H, W, Cout = 2, 7, 9, 48
    K = k * k * cin
    must = sorted({0, 15, 16, K - 1, K - 16, K - 17, K - 33} | {t * cin for t in range(k * k)} |
                  {t * cin + cin - 1 for t in range(k * k)})
    ks = (must + [v for v in sorted({int(v) for v in np.linspace(0, K - 1, 97)}) if v not in must])[:Cout]
    assert len(ks) == Cout == len(set(ks))
    w = np.zeros((Cout, K), np.int8)
    for co, kk in enumerate(ks):
        w[co, kk] = 1 + co % 3
    w = w.reshape(Cout, k, k, cin)
    x = np.zeros((B, H, W, cin), np.int8)
    x[1, 3, 4] = 1 + np.arange(cin) % 100
    acc = S.sums(x, w, k, stride)
    assert (acc != 0).any()
    if stride == 1:
        assert all(np.count_nonzero(acc[..., co]) == 1 for co in range(Cout))
    got = c_call(Arena(CAPACITY, POISONS[0]), x, w, None, None, None, NONE, stride, "slice", "fp16", scale_a=1.0)
    _assert_equal(got, acc.astype(np.float16))


# ---------------------------------------------------------------------------------------------- tail isolation
@pytest.mark.parametrize("cin,k", [(96, 3), (160, 1), (32, 1), (32, 3)])
@pytest.mark.parametrize("poison", POISONS)
def test_tail_chunks_read_nothing_behind_the_row(cin, k, poison):
    """K % 64 != 0: the last step of a row is half empty, and behind row co's K values lies row co + 1.  Even rows are
    all 127, odd rows all zero, x is all 127: an odd output channel is 0 unless the tail chunk of its row read the next
    row -- and the last row (odd) is followed by the arena's poison (-1 or 85 as int8)."""
    B, H, W, Cout = 1, 7, 9, 48
    assert (k * k * cin) % 64 != 0
    w = np.zeros((Cout, k, k, cin), np.int8)
    w[0::2] = 127
    x = np.full((B, H, W, cin), 127, np.int8)
    acc = S.sums(x, w, k, 1)
    assert not acc[..., 1::2].any() and acc[..., 0::2].all()
    s = 2.0 ** -12
    got = c_call(Arena(CAPACITY, poison), x, w, None, None, None, NONE, 1, "dense", "fp16", scale_a=s)
    _assert_equal(got, S.exact_output(acc, s, 1.0, None, None, NONE, None, 1.0, None, "fp16"))
    assert not got[..., 1::2].any()


# ---------------------------------------------------------------------------------------------- SiLU, general scales
# (B, H, W, Cin, Cout, ksize, stride, layout)
SILU_CASES = ((2, 7, 9, 96, 48, 3, 1, "slice"), (1, 12, 11, 160, 144, 1, 1, "same"), (2, 12, 11, 32, 64, 3, 2, "inplace"))


@functools.lru_cache(maxsize=None)
def silu_case(case):
    B, H, W, Cin, Cout, k, stride, _ = case
    r = X._rng("conv_slice_s8 silu", case)
    x = np.clip(np.rint(r.normal(0, 40, (B, H, W, Cin))), -127, 127).astype(np.int8)
    w = np.clip(np.rint(r.normal(0, 40, (Cout, k, k, Cin))), -127, 127).astype(np.int8)
    scale_a, scale_res = np.float32(0.0371), np.float32(0.0433)
    # pre-activations of a standard deviation around 3: SiLU's curved part
    ws = (r.uniform(0.5, 2.0, Cout) * 3.0 / (40.0 * 40.0 * np.sqrt(k * k * Cin) * float(scale_a))).astype(np.float32)
    bias = r.normal(0, 1, Cout).astype(np.float32)
    Ho, Wo = X.conv_out_hw(H, W, k, stride)
    res = np.clip(np.rint(r.normal(0, 40, (B, Ho, Wo, Cout))), -127, 127).astype(np.int8)
    acc = S.sums(x, w, k, stride)
    return x, w, ws, bias, res, acc, scale_a, scale_res


@pytest.mark.parametrize("identity", [False, True], ids=["plain", "identity"])
@pytest.mark.parametrize("case", SILU_CASES, ids=lambda c: "x".join(map(str, c)))
def test_silu_general_scales_within_the_derived_interval(case, identity):
    x, w, ws, bias, res, acc, scale_a, scale_res = silu_case(case)
    layout = case[7]
    if layout == "inplace" and not identity:
        layout = "slice"                         # (out identical to the identity needs an identity)
    r = res if identity else None
    t0, _, _, _ = S.silu_interval(acc, scale_a, 1.0, ws, bias, r, scale_res, 1.0)
    scale_out = np.float32(t0.std() / 47.3)                    # outputs on both sides of the clamp; no power of two
    t, delta, lo, hi = S.silu_interval(acc, scale_a, 1.0, ws, bias, r, scale_res, scale_out)
    assert (np.abs(t) > 127.5).any() and delta.max() < 0.01
    runs = [run_both_poisons(x, w, ws, bias, r, SILU, case[6], layout, "int8", scale_a=float(scale_a),
                             scale_res=float(scale_res), scale_out=float(scale_out)) for _ in range(2)]
    assert np.array_equal(runs[0], runs[1]), "two runs differ"
    share = S.check_interval(runs[0], lo, hi)
    off = float((runs[0] != np.clip(np.rint(t), -127, 127)).mean())
    print(f"delta max {delta.max():.2e} steps; {share:.4%} of the outputs within delta of a half-integer; {off:.4%} differ "
          f"from rne(t)")


# ---------------------------------------------------------------------------------------------- the existing kernel
@pytest.mark.parametrize("act", [NONE, RELU], ids=["linear", "relu"])
@pytest.mark.parametrize("out", ["int8", "fp16"])
@pytest.mark.parametrize("case", [(2, 12, 11, 64, 144, 3, 1), (1, 7, 9, 64, 16, 1, 2), (2, 7, 9, 128, 48, 3, 2)],
                         ids=lambda c: "x".join(map(str, c)))
def test_equals_conv_tile_int8(case, out, act):
    """pitch == channels, no identity, act in {none, ReLU}, Cin % 64 == 0, the power-of-two operands: the bytes of
    bevops_conv_tile_int8."""
    B, H, W, Cin, Cout, k, stride = case
    L, h, st = _lib()
    r = X._rng("conv_slice_s8 vs tile", case)
    x = X.gen_int8(r, (B, H, W, Cin))
    w, ws = X.gen_weights_int8(r, Cout, k * k * Cin, True)
    w = w.reshape(Cout, k, k, Cin)
    bias = X.gen_bias(r, Cout, "s8")
    s_out = 2.0 ** -3
    got = c_call(Arena(CAPACITY, POISONS[1]), x, w, ws, bias, None, act, stride, "dense", out, scale_out=s_out)
    dev = torch.device("cuda")
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    wsd, bd = torch.from_numpy(ws).to(dev), torch.from_numpy(bias).to(dev)
    ref = torch.empty(got.shape, dtype=torch.int8 if out == "int8" else torch.float16, device=dev)
    rc = h.bevops_conv_tile_int8(xd.data_ptr(), S_A, wd.data_ptr(), wsd.data_ptr(), 1.0, bd.data_ptr(), None,
                                 L.I8 if out == "int8" else L.F16, ref.data_ptr(), s_out, B, H, W, Cin, Cout, k, stride,
                                 int(act == RELU), st)
    assert rc == L.SUCCESS
    _assert_equal(got, ref.cpu().numpy())
    assert got.any()


# ---------------------------------------------------------------------------------------------- non-finite, int32
@pytest.mark.parametrize("out", ["int8", "fp16"])
@pytest.mark.parametrize("act", [NONE, SILU], ids=["linear", "silu"])
def test_non_finite_bias_stays_in_its_channel(act, out):
    """A NaN / +inf / -inf bias touches only its own output channel.  int8: the clamp's value -- NaN -> -127
    (max(NaN, -127) = -127), +inf -> 127, -inf -> -127 (and SiLU(-inf) = -inf * 0 = NaN -> -127); fp16: the value goes
    through as it is (SiLU(-inf): NaN)."""
    case = (2, 7, 9, 96, 48, 3, 1, "slice")
    x, w, ws, bias, res, acc, scale_a, scale_res = silu_case(case)
    args = dict(scale_a=float(scale_a), scale_res=float(scale_res), scale_out=0.11)
    clean = c_call(Arena(CAPACITY, POISONS[0]), x, w, ws, bias, res, act, 1, "slice", out, **args)
    bad = bias.copy()
    bad[5], bad[17], bad[40] = np.nan, np.inf, -np.inf
    got = c_call(Arena(CAPACITY, POISONS[0]), x, w, ws, bad, res, act, 1, "slice", out, **args)
    others = np.ones(48, bool)
    others[[5, 17, 40]] = False
    assert np.array_equal(_bits(got[..., others]), _bits(clean[..., others]))
    if out == "int8":
        assert (got[..., 5] == -127).all() and (got[..., 17] == 127).all() and (got[..., 40] == -127).all()
    else:
        assert np.isnan(got[..., 5]).all() and np.isposinf(got[..., 17]).all()
        assert np.isnan(got[..., 40]).all() if act == SILU else np.isneginf(got[..., 40]).all()


def test_int32_sums_cannot_overflow_at_the_largest_k():
    """|sum| <= K * 127 * 127; the largest K of these tests (and of YOLOX-x: 9 * 1280 = 11 520 -> 1.86e8) is far below
    2^31 / 16 129 = 133 143.  All -127 inputs on all -127 weights at K = 9 * 160: 23 225 760 at interior pixels."""
    B, H, W, Cin, Cout, k = 1, 7, 9, 160, 16, 3
    x = np.full((B, H, W, Cin), -127, np.int8)
    w = np.full((Cout, k, k, Cin), -127, np.int8)
    acc = S.sums(x, w, k, 1)
    assert acc.max() == 9 * 160 * 127 * 127 == 23225760 and 11520 * 16129 < 2 ** 31
    s = 2.0 ** -12
    got = c_call(Arena(CAPACITY, POISONS[0]), x, w, None, None, None, NONE, 1, "dense", "fp16", scale_a=s)
    _assert_equal(got, S.exact_output(acc, s, 1.0, None, None, NONE, None, 1.0, None, "fp16"))
