"""CPU-only: the pre-launch status contract of bevops_conv_slice_s8 (csrc/conv_slice_s8.hip) and of the three int8 entries
of csrc/yolox.hip, `slice_pitch` on int8 views, and the per-channel weight quantisation of
functions.yolox_ops.quantize_weight_taps against a float64 statement."""
import ctypes

import numpy as np
import pytest
import torch

SUCCESS, BAD_PARAM, NOT_SUPPORTED = 0, 2, 3
F16, I8 = 1, 2


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_char * 8192)()
    addr = (ctypes.addressof(buf) + 255) & ~255          # aligned host address: never dereferenced
    return addr, buf


def test_dtype_codes():
    from bevformer_tensorrt_amd.utils import lib as L
    assert (L.F16, L.I8) == (F16, I8)


def test_symbols_resolve_and_are_exported(lib):
    import bevformer_tensorrt_amd as bev
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.utils.lib import SIGNATURES
    for name in ("bevops_conv_slice_s8", "bevops_focus_nhwc_q", "bevops_spp_maxpool_nhwc_s8",
                 "bevops_upsample_nearest2x_nhwc_s8"):
        assert name in SIGNATURES
        assert lib.bevops_query(name.encode()) == ctypes.cast(getattr(lib, name), ctypes.c_void_p).value, name
    for name in ("conv_slice_q_taps", "focus_nhwc_q", "quantize_weight_taps"):
        assert name in fn.__all__ and getattr(bev, name) is getattr(fn, name)
        assert name not in bev.TRT_FUNCTIONS


def test_conv_slice_s8_status_codes_without_gpu(lib, p):
    p = p[0]
    inf, nan = float("inf"), float("nan")

    def call(x=p, xp=32, sa=0.5, w=p + 256, ws=p + 512, sw=1.0, b=p + 1024, r=None, rp=0, sr=1.0, od=I8, o=p + 2048, op=16,
             so=0.25, B=1, H=4, W=4, Cin=32, Cout=16, ks=3, s=1, act=2):
        return lib.bevops_conv_slice_s8(x, xp, sa, w, ws, sw, b, r, rp, sr, od, o, op, so, B, H, W, Cin, Cout, ks, s, act,
                                        None)

    res = p + 4096
    # outside the domain: Cin % 32 (NOT 64: 32, 96 and 160 are inside), Cout % 16 (int8 out) / % 8 (fp16 out)
    assert call(Cin=48, xp=48) == NOT_SUPPORTED and call(Cin=16, xp=16) == NOT_SUPPORTED
    assert call(Cout=24, op=32) == NOT_SUPPORTED and call(Cout=8, op=16) == NOT_SUPPORTED
    assert call(Cout=12, op=16, od=F16) == NOT_SUPPORTED
    assert call(ks=5) == NOT_SUPPORTED and call(ks=2) == NOT_SUPPORTED and call(s=3) == NOT_SUPPORTED
    assert call(act=3) == NOT_SUPPORTED and call(act=-1) == NOT_SUPPORTED
    assert call(od=0) == NOT_SUPPORTED and call(od=3) == NOT_SUPPORTED
    # bad parameters
    assert call(H=0) == BAD_PARAM and call(W=-1) == BAD_PARAM and call(B=-1) == BAD_PARAM
    assert call(Cin=0) == BAD_PARAM and call(Cout=0) == BAD_PARAM and call(ks=0) == BAD_PARAM and call(s=0) == BAD_PARAM
    assert call(x=None) == BAD_PARAM and call(w=None) == BAD_PARAM and call(o=None) == BAD_PARAM
    assert call(x=p + 8) == BAD_PARAM and call(w=p + 264) == BAD_PARAM and call(o=p + 2056) == BAD_PARAM
    assert call(r=res + 8, rp=16) == BAD_PARAM and call(b=p + 1026) == BAD_PARAM and call(ws=p + 513) == BAD_PARAM
    assert call(xp=16) == BAD_PARAM and call(op=0) == BAD_PARAM and call(r=res, rp=0) == BAD_PARAM      # pitch < channels
    assert call(xp=40) == BAD_PARAM and call(op=24) == BAD_PARAM and call(r=res, rp=24) == BAD_PARAM    # pitch % 16
    assert call(od=F16, Cout=8, op=12) == BAD_PARAM                                                    # fp16 out: pitch % 8
    # a scale in use is positive and finite
    for bad in (0.0, -1.0, inf, nan):
        assert call(sa=bad) == BAD_PARAM and call(sw=bad) == BAD_PARAM and call(so=bad) == BAD_PARAM
        assert call(r=res, rp=16, sr=bad) == BAD_PARAM
        assert call(B=0, sr=bad) == SUCCESS                       # no identity: scale_res is not in use
        assert call(B=0, od=F16, so=bad) == SUCCESS               # fp16 out: scale_out is not in use
    # nothing to do; the widths of YOLOX-x; optional operands
    assert call(B=0) == SUCCESS and call(B=0, b=None, ws=None) == SUCCESS
    assert call(B=0, r=res, rp=16, xp=64, op=48) == SUCCESS
    for cin in (32, 64, 96, 160):
        assert call(B=0, Cin=cin, xp=cin) == SUCCESS
    assert call(B=0, od=F16, Cout=88, op=88) == SUCCESS
    # x is addressed through 32-bit byte offsets: B H W x_pitch of 0xFFFFFF00 bytes and more are refused
    assert call(B=1, H=65536, W=2048, Cin=32) == NOT_SUPPORTED                 # 2^32 bytes
    assert call(B=1, H=65536, W=1024, Cin=32, xp=64) == NOT_SUPPORTED          # the pitch counts, not the channels


def test_int8_yolox_entries_status_codes_without_gpu(lib, p):
    p = p[0]

    def focus(img=p, s=0.5, o=p + 256, op=32, B=1, H=4, W=4):
        return lib.bevops_focus_nhwc_q(img, s, o, op, B, H, W, None)

    assert focus(H=3) == NOT_SUPPORTED and focus(W=5) == NOT_SUPPORTED
    assert focus(img=None) == BAD_PARAM and focus(o=None) == BAD_PARAM and focus(o=p + 264) == BAD_PARAM
    assert focus(img=p + 1) == BAD_PARAM and focus(op=16) == BAD_PARAM and focus(op=40) == BAD_PARAM
    assert focus(H=0) == BAD_PARAM and focus(B=-1) == BAD_PARAM
    assert focus(s=0.0) == BAD_PARAM and focus(s=float("nan")) == BAD_PARAM and focus(s=float("inf")) == BAD_PARAM
    assert focus(B=0) == SUCCESS
    assert focus(H=131072, W=131072) == NOT_SUPPORTED

    def spp(x=p, xp=16, o=p + 256, op=48, B=1, H=4, W=4, C=16, k=(5, 9, 13)):
        return lib.bevops_spp_maxpool_nhwc_s8(x, xp, o, op, B, H, W, C, *k, None)

    assert spp(C=8, xp=16, op=48) == NOT_SUPPORTED and spp(C=24, xp=32, op=80) == NOT_SUPPORTED
    assert spp(k=(4, 9, 13)) == NOT_SUPPORTED and spp(k=(5, 9, 15)) == NOT_SUPPORTED
    assert spp(k=(0, 9, 13)) == BAD_PARAM
    assert spp(x=None) == BAD_PARAM and spp(o=None) == BAD_PARAM and spp(x=p + 8) == BAD_PARAM and spp(o=p + 260) == BAD_PARAM
    assert spp(xp=8) == BAD_PARAM and spp(op=32) == BAD_PARAM and spp(op=56) == BAD_PARAM   # out holds three slices
    assert spp(W=0) == BAD_PARAM and spp(C=0) == BAD_PARAM
    assert spp(B=0) == SUCCESS
    assert spp(H=65536, W=65536) == NOT_SUPPORTED

    def up(x=p, xp=16, o=p + 256, op=16, B=1, H=4, W=4, C=16):
        return lib.bevops_upsample_nearest2x_nhwc_s8(x, xp, o, op, B, H, W, C, None)

    assert up(C=8, xp=16, op=16) == NOT_SUPPORTED
    assert up(x=None) == BAD_PARAM and up(o=None) == BAD_PARAM and up(x=p + 2) == BAD_PARAM and up(o=p + 264) == BAD_PARAM
    assert up(xp=0) == BAD_PARAM and up(op=8) == BAD_PARAM and up(op=24) == BAD_PARAM and up(H=-1) == BAD_PARAM
    assert up(B=0) == SUCCESS
    assert up(H=32768, W=32768) == NOT_SUPPORTED


def test_slice_pitch_on_int8_views():
    from bevformer_tensorrt_amd.functions.yolox_ops import nhwc_empty, slice_pitch
    buf = nhwc_empty(2, 64, 3, 5, "cpu", torch.int8)
    assert buf.dtype == torch.int8 and slice_pitch(buf) == 64
    assert slice_pitch(buf[:, 16:48]) == 64 and slice_pitch(buf[:, 48:]) == 64
    with pytest.raises(ValueError, match="multiple of 16 elements"):
        slice_pitch(buf[:, 8:24])                                  # 8 bytes into the pixel: no 16-byte boundary
    with pytest.raises(ValueError, match="multiple of 16 elements"):
        slice_pitch(nhwc_empty(1, 24, 2, 2, "cpu", torch.int8))    # pitch 24
    with pytest.raises(ValueError, match="not a channel slice"):
        slice_pitch(torch.empty((2, 32, 3, 5), dtype=torch.int8))  # planar
    assert slice_pitch(nhwc_empty(1, 16, 1, 1, "cpu", torch.int8)) == 16
    # the fp16 rule is unchanged: 8 elements
    half = nhwc_empty(1, 24, 2, 2, "cpu")
    assert slice_pitch(half) == 24 and slice_pitch(half[:, 8:16]) == 24
    with pytest.raises(ValueError, match="multiple of 8 elements"):
        slice_pitch(nhwc_empty(1, 12, 2, 2, "cpu"))


@pytest.mark.parametrize("shape,groups_in", [((80, 160, 3, 3), (80, 80)), ((80, 12, 3, 3), None), ((64, 32, 1, 1), None)])
def test_weight_quantisation_is_the_float64_statement(shape, groups_in):
    """scale[co] = fp32(amax_co) / 127 in fp32, q = clamp(rne(fp32(w / scale)), -127, 127): stated in numpy with every
    fp32 rounding explicit; pad rows scale 1 and zero weights, pad columns zero, pad bias zero."""
    from bevformer_tensorrt_amd.functions.yolox_ops import pad_channels, quantize_weight_taps
    g = torch.Generator().manual_seed(sum(shape))
    w = (torch.randn(shape, generator=g) * 0.1).half()
    b = torch.randn((shape[0],), generator=g).half()
    q, s, bias = quantize_weight_taps(w, b, groups_in=groups_in)
    wp, bp = pad_channels(w.float(), b.float(), groups_in=groups_in)
    wp64 = wp.numpy().astype(np.float64)
    amax = np.abs(wp64).max(axis=(1, 2, 3))
    want_s = np.where(amax > 0, (amax.astype(np.float32) / np.float32(127.0)).astype(np.float32), np.float32(1.0))
    assert s.dtype == torch.float32 and np.array_equal(s.numpy(), want_s)
    quot = (wp64 / want_s.astype(np.float64)[:, None, None, None]).astype(np.float32)    # the fp32 quotient
    want_q = np.clip(np.rint(quot.astype(np.float64)), -127, 127).astype(np.int8)
    assert q.dtype == torch.int8 and q.is_contiguous() and tuple(q.shape) == (wp.shape[0], shape[2], shape[3], wp.shape[1])
    assert np.array_equal(q.numpy(), np.transpose(want_q, (0, 2, 3, 1)))
    assert bias.dtype == torch.float32 and np.array_equal(bias.numpy(), bp.numpy())
    real = shape[0]
    assert int(np.abs(q.numpy()[:real]).max(axis=(1, 2, 3)).min()) == 127         # every real row uses the whole range
    if wp.shape[0] > real:
        assert not q[real:].any() and not bias[real:].any() and bool((s[real:] == 1).all())
    assert not q.numpy()[..., ~(np.abs(wp64).max(axis=(0, 2, 3)) > 0)].any()       # pad columns
