"""CPU-only: bevops_deform_conv3x3_nhwc_s8, the INT8 form of the DepthNet's DCN layer (design/bevdepth_dcn_int8.md).

Every pre-launch status of the entry in the order include/bevops.h states, the wrapper's first errors (the rest need a
device: tests/test_deform_conv_s8_gpu.py), the float64 / numpy statement of tests/util_deform_conv_s8.py on its own --
zero offsets reduce it to a plain grouped convolution, integer offsets are shifted taps, a NaN / +-inf / 60 000 offset
kills exactly its tap -- and the premises of the GPU tests computed from the statement alone: the lattice claims, the
near-tie shares of the general-offset cases under their cap, the general-scale interval's share under its cap."""
import ctypes

import numpy as np
import pytest
import torch

import util_conv_slice_s8 as S
import util_deform_conv_s8 as D
import util_exact_dense as X

SUCCESS, BAD_PARAM, NOT_SUPPORTED = 0, 2, 3
F32, F16, I8 = 0, 1, 2
NAME = "bevops_deform_conv3x3_nhwc_s8"


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_char * 8192)()
    return (ctypes.addressof(buf) + 255) & ~255, buf          # aligned host address: never dereferenced


def test_symbol_resolves_and_is_exported(lib):
    import bevformer_tensorrt_amd as bev
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.utils.lib import SIGNATURES
    assert NAME in SIGNATURES and getattr(lib, NAME).argtypes == SIGNATURES[NAME][1]
    assert lib.bevops_query(NAME.encode()) == ctypes.cast(getattr(lib, NAME), ctypes.c_void_p).value
    f = "deform_conv2d_q_nhwc"
    assert f in fn.__all__ and getattr(bev, f) is getattr(fn, f) and f not in bev.TRT_FUNCTIONS


def test_status_codes_in_the_documented_order(lib, p):
    p = p[0]
    inf, nan = float("inf"), float("nan")

    def call(x=p, xp=128, sa=0.5, off=p + 256, oc=24, w=p + 512, ws=p + 768, sw=1.0, b=None, od=I8, out=p + 1024, op=128,
             so=0.25, relu=0, B=1, H=4, W=5, cin=128, cout=128, g=4):
        return getattr(lib, NAME)(x, xp, sa, off, oc, w, ws, sw, b, od, out, op, so, relu, B, H, W, cin, cout, g, None)

    assert call(B=0) == SUCCESS
    # BAD_PARAM: pointers
    for k in ("x", "off", "w", "out"):
        assert call(**{k: None}) == BAD_PARAM, k
        assert call(**{k: p + 2048 + 8}) == BAD_PARAM, k
    assert call(ws=p + 2048 + 4) == BAD_PARAM and call(b=p + 2048 + 8) == BAD_PARAM
    assert call(B=0, ws=None) == SUCCESS and call(B=0, b=p + 2048) == SUCCESS
    # sizes, relu, the offset rows
    assert call(B=-1) == BAD_PARAM and call(H=0) == BAD_PARAM and call(W=0) == BAD_PARAM
    assert call(cin=0) == BAD_PARAM and call(cout=0) == BAD_PARAM and call(g=0) == BAD_PARAM and call(g=-4) == BAD_PARAM
    assert call(relu=2) == BAD_PARAM and call(relu=-1) == BAD_PARAM
    assert call(oc=16) == BAD_PARAM and call(oc=19) == BAD_PARAM and call(oc=0) == BAD_PARAM
    assert call(B=0, oc=18) == SUCCESS and call(B=0, oc=32) == SUCCESS
    # pitches: int8 slices in 16-element steps, fp16 out in 8-element steps
    assert call(xp=112) == BAD_PARAM and call(xp=136) == BAD_PARAM and call(B=0, xp=144) == SUCCESS
    assert call(op=112) == BAD_PARAM and call(op=136) == BAD_PARAM and call(B=0, op=144) == SUCCESS
    assert call(B=0, od=F16, op=136) == SUCCESS
    assert call(od=F16, op=132) == BAD_PARAM and call(od=F16, op=120) == BAD_PARAM
    # scales in use
    for bad in (0.0, -1.0, inf, nan):
        assert call(sa=bad) == BAD_PARAM and call(sw=bad) == BAD_PARAM and call(so=bad) == BAD_PARAM, bad
        assert call(B=0, od=F16, so=bad) == SUCCESS, bad                     # not in use with fp16 out
    # NOT_SUPPORTED behind every parameter check, answered for an empty batch too
    assert call(od=F32) == NOT_SUPPORTED and call(od=3) == NOT_SUPPORTED and call(od=F32, B=0) == NOT_SUPPORTED
    assert call(od=F32, relu=2) == BAD_PARAM and call(od=F32, sa=0.0) == BAD_PARAM and call(od=F32, op=120) == BAD_PARAM
    assert call(cin=144, xp=144) == NOT_SUPPORTED and call(cout=144, op=144) == NOT_SUPPORTED         # % groups, % 32
    assert call(cin=64, xp=64) == NOT_SUPPORTED and call(cout=64, op=64) == NOT_SUPPORTED
    assert call(cin=192, xp=192, g=4) == NOT_SUPPORTED and call(cin=64, xp=64, B=0) == NOT_SUPPORTED
    assert call(cin=64, xp=64, oc=16) == BAD_PARAM and call(cin=64, xp=64, x=None) == BAD_PARAM
    # size limits: the 32-bit pixel index, the grid's row count
    assert call(B=1 << 15, H=1 << 8, W=1 << 8) == NOT_SUPPORTED
    assert call(B=1, H=1 << 16, W=1 << 16) == NOT_SUPPORTED
    big = 32 * 65536
    assert call(B=0, cin=big, xp=big, cout=big, op=big, g=65536) == NOT_SUPPORTED
    # an empty batch inside the domain: success, nothing launched (no device is needed)
    assert call(B=0, cin=32, xp=32, cout=32, op=32, g=1) == SUCCESS and call(B=0, cin=256, xp=256, g=4) == SUCCESS
    assert call(B=0, cin=192, xp=192, cout=192, op=192, g=2, relu=1, od=F16) == SUCCESS


def test_wrapper_refuses_host_tensors():
    from bevformer_tensorrt_amd.functions import deform_conv2d_q_nhwc
    x = torch.zeros(1, 32, 2, 2, dtype=torch.int8)
    off = torch.zeros(1, 24, 2, 2, dtype=torch.float16)
    w = torch.zeros(32, 3, 3, 32, dtype=torch.int8)
    with pytest.raises(TypeError, match="int8 CUDA"):
        deform_conv2d_q_nhwc(x, 1.0, off, w, None, None, 1, scale_out=1.0)
    with pytest.raises(TypeError, match="int8 CUDA"):
        deform_conv2d_q_nhwc(x.float(), 1.0, off, w, None, None, 1, scale_out=1.0)


def test_cpu_statement_keeps_its_bits_and_takes_a_column_hook():
    """_deform_conv2d_cpu: the column hook sees [B, Cin, 9, Ho, Wo]; the identity hook changes nothing."""
    from bevformer_tensorrt_amd.functions.deform_conv import _deform_conv2d_cpu, deform_conv2d
    g = torch.Generator().manual_seed(5)
    x, off = torch.randn(2, 64, 4, 5, generator=g), torch.randn(2, 18, 4, 5, generator=g)
    w = torch.randn(64, 16, 3, 3, generator=g)
    want = deform_conv2d(x, off, w, 1, 1, 1, 4, 1)
    seen = []
    got = _deform_conv2d_cpu(x, off, w, 1, 1, 1, 4, 1, column=lambda c: (seen.append(tuple(c.shape)), c)[1])
    assert torch.equal(got, want) and seen == [(2, 64, 9, 4, 5)]
    zero = _deform_conv2d_cpu(x, off, w, 1, 1, 1, 4, 1, column=torch.zeros_like)
    assert float(zero.abs().max()) == 0.0


# ---- the statement's own properties

def _plain_sums(x, w, groups):
    cin_g, cout = w.shape[3], w.shape[0]
    cout_g = cout // groups
    B, H, W, _ = x.shape
    out = np.empty((B, H, W, cout), np.int64)
    for g in range(groups):
        out[..., g * cout_g:(g + 1) * cout_g] = S.sums(x[..., g * cin_g:(g + 1) * cin_g], w[g * cout_g:(g + 1) * cout_g], 3, 1)
    return out


@pytest.mark.parametrize("ch", [(32, 32, 1), (64, 64, 4), (96, 32, 2)], ids=str)
def test_zero_offsets_are_a_plain_grouped_convolution(ch):
    x, _, w, _, _, _, _ = D.lattice_case(ch, D.PIXELS[1])
    off = np.zeros(x.shape[:3] + (18,), np.float16)
    s64 = D.column_s64(x, off)
    assert np.array_equal(s64, np.rint(s64))
    assert np.array_equal(D.sums(D.column(s64), w, ch[2]), _plain_sums(x, w, ch[2]))


def test_integer_offsets_are_shifted_taps():
    ch = (32, 32, 1)
    x, _, w, _, _, _, _ = D.lattice_case(ch, D.PIXELS[1])
    B, H, W, C = x.shape
    for dy, dx in ((0, 1), (-1, 0), (2, -3)):
        off = np.zeros((B, H, W, 18), np.float16)
        off[..., 0::2], off[..., 1::2] = dy, dx
        shifted = np.zeros_like(x)
        ys, xs = np.arange(H), np.arange(W)
        vy, vx = (ys + dy >= 0) & (ys + dy < H), (xs + dx >= 0) & (xs + dx < W)
        shifted[:, ys[vy][:, None], xs[vx][None, :]] = x[:, (ys + dy)[vy][:, None], (xs + dx)[vx][None, :]]
        # a tap whose shifted position lies outside the image reads zero in both statements; the PLAIN convolution of
        # the shifted image also zero-pads at ITS border, where the deformable one reads real pixels of x: compare the
        # pixels whose nine un-shifted taps are inside the image
        got = D.sums(D.column(D.column_s64(x, off)), w, 1)
        want = _plain_sums(shifted, w, 1)
        assert np.array_equal(got[:, 1:H - 1, 1:W - 1], want[:, 1:H - 1, 1:W - 1]), (dy, dx)
        assert not np.array_equal(got, _plain_sums(x, w, 1))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf"), 60000.0], ids=str)
def test_non_finite_and_huge_offsets_kill_exactly_their_tap(bad):
    ch = (32, 32, 1)
    x, off, w, _, _, s64, _ = D.lattice_case(ch, D.PIXELS[1])
    b, y, xx, tap = 1, 4, 7, 5
    for comp in (0, 1):
        o = np.array(off)
        o[b, y, xx, 2 * tap + comp] = bad
        s = D.column_s64(x, o)
        assert np.isfinite(s).all()
        assert float(np.abs(s[b, y, xx, tap]).max()) == 0.0
        keep = np.ones(s.shape[:4], bool)
        keep[b, y, xx, tap] = False
        assert np.array_equal(s[keep], s64[keep])
    assert float(np.abs(s64[b, y, xx, tap]).max()) > 0.0                       # the tap was live before


# ---- the premises of the GPU tests, from the statement alone

@pytest.mark.parametrize("ch", D.CHANNELS, ids=str)
def test_lattice_premises(ch):
    """On the lattice every blend is a multiple of 2^-12 below 128 (the fp32 chain is exact), true ties occur, the sums
    stay below 2^24, and the exact epilogue leaves ties and both saturations."""
    x, off, w, ws, bias, s64, acc = D.lattice_case(ch, D.PIXELS[1])
    assert np.array_equal(s64 * 4096, np.rint(s64 * 4096)) and np.abs(s64).max() <= 127
    _, wgt, live = D.positions(off, *x.shape[1:3])
    assert np.array_equal(wgt.astype(np.float64) * 4096, np.rint(wgt.astype(np.float64) * 4096))
    ties = float((np.abs(s64 - np.floor(s64) - 0.5) == 0).mean())
    dead = 1.0 - float(live.mean())
    print(f"{ch}: {ties:.3%} true ties of the blend, {dead:.1%} dead taps, max |sum| {np.abs(acc).max()}")
    assert ties > 1e-3 and 0.02 < dead < 0.6
    assert np.abs(acc).max() < 2 ** 24 and 9 * 96 * 127 ** 2 < 2 ** 24
    for relu in (0, 1):
        want, s_out, t = D.lattice_statement(ch, D.PIXELS[1], True, relu, "int8")
        t_ties, beyond = X.int8_shares(t)
        assert t_ties > 0 and beyond > 0 and (want == 127).any() and ((want == -127).any() or relu)
        got = S.exact_output(acc, D.S_A, 1.0, ws, bias, relu, None, 1.0, s_out, "int8")
        assert np.array_equal(got, want)
    want16, _, _ = D.lattice_statement(ch, D.PIXELS[1], True, 0, "fp16")
    assert np.array_equal(S.exact_output(acc, D.S_A, 1.0, ws, bias, 0, None, 1.0, 1.0, "fp16").view(np.int16), want16.view(np.int16))


@pytest.mark.parametrize("seed", D.GENERAL_SEEDS)
@pytest.mark.parametrize("ch", D.CHANNELS, ids=str)
def test_general_offset_cases_hold_their_near_tie_cap(ch, seed):
    _, _, w, picks, sel = D.general_case(ch, seed)
    assert (w.reshape(w.shape[0], -1) != 0).sum(axis=1).tolist() == [1] * w.shape[0] and len(picks) == w.shape[0]
    assert {t for t, _ in picks} == set(range(9))
    share = float(D.near_tie(sel).mean())
    lo, hi = D.column_interval(sel)
    print(f"{ch} seed {seed}: {share:.2e} of {sel.size} within EPS of a half-integer")
    assert share <= D.NEAR_TIE_CAP and float((lo != hi).mean()) <= D.NEAR_TIE_CAP
    assert (np.abs(sel) > 1).mean() > 0.3                                      # live, non-trivial columns


@pytest.mark.parametrize("ch", D.CHANNELS, ids=str)
def test_general_scale_interval_holds_its_share_cap(ch):
    _, _, _, _, _, _, acc = D.lattice_case(ch, D.PIXELS[1])
    ws, bias, s_out = D.general_scale_operands(ch)
    for relu in (0, 1):
        t, delta, lo, hi = D.linear_interval(acc, D.GENERAL_S_A, 1.0, ws, bias, relu, s_out)
        want = S.exact_output(acc, D.GENERAL_S_A, 1.0, ws, bias, relu, None, 1.0, s_out, "int8")
        share = S.check_interval(want, lo, hi)
        print(f"{ch} relu {relu}: {share:.2e} excused, max delta {delta.max():.2e} steps")
        assert (np.abs(t) > 127).any() and delta.max() < 1e-3
