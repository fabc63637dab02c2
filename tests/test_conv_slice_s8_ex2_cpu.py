"""CPU-only: the pre-launch status contract of bevops_conv_slice_s8_ex2 (csrc/conv_slice_s8.hip) in the order
include/bevops.h states, and the properties of the statements tests/test_conv_slice_s8_ex2_gpu.py compares with: the
dilated integer sums against a float64 F.conv2d(dilation=), and the lattice statements' exactness."""
import ctypes

import numpy as np
import pytest
import torch

import util_conv_slice_s8_ex2 as E
import util_exact_dense as X

SUCCESS, BAD_PARAM, NOT_SUPPORTED = 0, 2, 3
F16, I8 = 1, 2


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_char * 16384)()
    addr = (ctypes.addressof(buf) + 255) & ~255          # aligned host address: never dereferenced
    return addr, buf


def test_symbol_resolves(lib):
    from bevformer_tensorrt_amd.utils.lib import SIGNATURES
    name = "bevops_conv_slice_s8_ex2"
    assert name in SIGNATURES
    assert lib.bevops_query(name.encode()) == ctypes.cast(getattr(lib, name), ctypes.c_void_p).value


def test_status_codes_without_gpu(lib, p):
    p = p[0]
    inf, nan = float("inf"), float("nan")
    res, ib = p + 4096, p + 8192

    def call(x=p, xp=32, sa=0.5, w=p + 256, ws=p + 512, sw=1.0, b=None, r=None, rp=0, sr=1.0, od=I8, o=p + 2048, op=16,
             so=0.25, B=1, H=4, W=4, Cin=32, Cout=16, ks=3, s=1, act=1, rf=0, d=1, ib=None, ibp=0):
        return lib.bevops_conv_slice_s8_ex2(x, xp, sa, w, ws, sw, b, r, rp, sr, od, o, op, so, B, H, W, Cin, Cout, ks, s, act,
                                            rf, d, ib, ibp, None)

    bias = p + 1024
    # everything BAD_PARAM of bevops_conv_slice_s8: NULL pointers, sizes, pitches, alignments, scales
    assert call(x=None) == BAD_PARAM and call(w=None) == BAD_PARAM and call(o=None) == BAD_PARAM
    assert call(H=0) == BAD_PARAM and call(B=-1) == BAD_PARAM and call(Cin=0) == BAD_PARAM and call(ks=0) == BAD_PARAM
    assert call(xp=16) == BAD_PARAM and call(xp=40) == BAD_PARAM and call(op=24) == BAD_PARAM
    assert call(r=res, rp=0) == BAD_PARAM and call(r=res, rp=24) == BAD_PARAM
    assert call(x=p + 8) == BAD_PARAM and call(w=p + 264) == BAD_PARAM and call(o=p + 2056) == BAD_PARAM
    assert call(b=bias + 2) == BAD_PARAM and call(ws=p + 513) == BAD_PARAM and call(r=res + 8, rp=16) == BAD_PARAM
    for bad in (0.0, -1.0, inf, nan):
        assert call(sa=bad) == BAD_PARAM and call(sw=bad) == BAD_PARAM and call(so=bad) == BAD_PARAM
        assert call(r=res, rp=16, sr=bad) == BAD_PARAM
    # dilation < 1
    assert call(d=0) == BAD_PARAM and call(d=-3) == BAD_PARAM and call(d=0, B=0) == BAD_PARAM
    assert call(d=0, ks=1) == BAD_PARAM                                       # in front of the domain checks
    # the per-image bias: not together with bias; its pitch and alignment
    assert call(ib=ib, ibp=16, b=bias) == BAD_PARAM
    assert call(ib=ib, ibp=8) == BAD_PARAM and call(ib=ib, ibp=0) == BAD_PARAM          # pitch < Cout
    assert call(ib=ib, ibp=20) == BAD_PARAM                                            # pitch % 8
    assert call(ib=ib + 8, ibp=16) == BAD_PARAM and call(ib=ib + 2, ibp=16) == BAD_PARAM
    assert call(ib=ib, ibp=20, ks=5) == BAD_PARAM                                     # in front of the domain checks
    assert call(ib=None, ibp=-5, B=0) == SUCCESS                                       # no image bias: its pitch is unused
    # everything NOT_SUPPORTED of bevops_conv_slice_s8_ex
    assert call(Cin=48, xp=48) == NOT_SUPPORTED and call(Cout=24, op=32) == NOT_SUPPORTED
    assert call(ks=5) == NOT_SUPPORTED and call(s=3) == NOT_SUPPORTED and call(act=3) == NOT_SUPPORTED
    assert call(od=0) == NOT_SUPPORTED
    assert call(rf=1) == NOT_SUPPORTED and call(rf=1, r=res, rp=16, act=2) == NOT_SUPPORTED
    # dilation > 1: ksize 3 and stride 1 only
    assert call(d=2, ks=1) == NOT_SUPPORTED and call(d=6, s=2) == NOT_SUPPORTED and call(d=2, ks=1, B=0) == NOT_SUPPORTED
    assert call(d=1, ks=1, B=0) == SUCCESS and call(d=1, s=2, B=0) == SUCCESS
    # the displacement of a tap is a signed 32-bit byte count: dilation (W + 1) x_pitch <= 0x7FFFFFFF
    # (computed for taps outside the image too), whatever B is
    assert call(d=1024, H=1, W=65535, xp=32, B=0) == NOT_SUPPORTED             # 2^10 2^16 2^5 = 2^31
    assert call(d=1023, H=1, W=65535, xp=32, B=0) == SUCCESS                   # 1023 2^21 < 2^31
    assert call(d=1, H=1, W=65535, xp=32768, Cin=32, B=0) == SUCCESS           # dilation 1 keeps bevops_conv_slice_s8's rule
    assert call(d=2, H=1, W=65535, xp=16384, Cin=32, B=0) == NOT_SUPPORTED     # 2 2^16 2^14 = 2^31
    # nothing to do
    assert call(B=0) == SUCCESS and call(B=0, d=18, ib=ib, ibp=16) == SUCCESS
    assert call(B=0, d=6, r=res, rp=16, rf=1) == SUCCESS and call(B=0, od=F16, Cout=88, op=88, ib=ib, ibp=88) == SUCCESS


@pytest.mark.parametrize("d", [1, 2, 6, 12, 18])
@pytest.mark.parametrize("shape", [(1, 5, 7, 32, 16), (3, 5, 7, 96, 48), (2, 16, 44, 64, 24)], ids=lambda s: "x".join(map(str, s)))
def test_dilated_integer_sums_are_float64_conv2d(shape, d):
    B, H, W, Cin, Cout = shape
    r = X._rng("ex2 sums", shape, d)
    x = X.gen_int8(r, (B, H, W, Cin))
    w = X.gen_int8(r, (Cout, 3, 3, Cin))
    got = E.sums_dilated(x, w, d)
    xt = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2)
    want = torch.nn.functional.conv2d(xt, wt, None, 1, d, d).permute(0, 2, 3, 1).numpy()
    assert got.dtype == np.int64 and np.array_equal(got.astype(np.float64), want) and got.any()
    if d == 1:
        import util_conv_slice_s8 as S
        assert np.array_equal(got, S.sums(x, w, 3, 1))


def test_the_taps_the_first_case_leaves_inside():
    """(1, 5, 7) at dilation 6: every tap with ky != 1 is outside; in columns 1 .. 5 every off-centre tap is."""
    x = np.ones((1, 5, 7, 32), np.int8)
    for ky in range(3):
        for kx in range(3):
            w = np.zeros((16, 3, 3, 32), np.int8)
            w[:, ky, kx] = 1
            hit = E.sums_dilated(x, w, 6)[0, :, :, 0] != 0
            if ky != 1:
                assert not hit.any()
            elif kx == 1:
                assert hit.all()
            else:
                assert not hit[:, 1:6].any() and hit[:, 0 if kx == 2 else 6].all()


@pytest.mark.parametrize("out", ["int8", "fp16"])
@pytest.mark.parametrize("epi", ["bias", "image"])
@pytest.mark.parametrize("case", E.LATTICE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_lattice_statement_is_exact_and_agrees_with_the_operation_order(case, epi, out):
    x, w, ws, bias, ibias, res, acc = E.operands(case)
    act = E.RELU if epi == "image" else E.NONE
    want, s_out, t = E.lattice_statement(case, epi, act, out)                # raises BudgetError off the lattice
    shared, per_image = (bias, None) if epi == "bias" else (None, ibias)
    got = E.order_statement(acc, E.S_A, ws, shared, per_image, act, None, 1.0, False, s_out, out)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)) and want.any()
    if t is not None:
        ties, beyond = X.int8_shares(t)
        assert ties > 0 and beyond > 0
