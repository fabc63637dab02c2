"""CPU-only: the pre-launch status contract of bevops_conv_slice_f16_ex (csrc/conv_slice.hip), in the order
include/bevops.h documents, and the argument checks of conv_slice_nhwc(dilation=, image_bias=) that need no device."""
import ctypes

import pytest

SUCCESS, BAD_PARAM, NOT_SUPPORTED = 0, 2, 3


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_char * 8192)()
    addr = (ctypes.addressof(buf) + 255) & ~255          # aligned host address: never dereferenced
    return addr, buf


def test_symbol_resolves_and_the_keywords_exist(lib):
    import inspect

    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.utils.lib import SIGNATURES
    name = "bevops_conv_slice_f16_ex"
    assert name in SIGNATURES
    assert lib.bevops_query(name.encode()) == ctypes.cast(getattr(lib, name), ctypes.c_void_p).value
    sig = inspect.signature(bev.conv_slice_nhwc)
    assert sig.parameters["dilation"].default == 1 and sig.parameters["image_bias"].default is None
    assert "conv_slice_nhwc" not in bev.TRT_FUNCTIONS


def test_status_codes_in_the_documented_order(lib, p):
    p = p[0]

    def call(x=p, xp=32, w=p + 256, b=p + 512, r=None, rp=0, o=p + 768, op=8, B=1, H=4, W=4, Cin=32, Cout=8, ks=3, s=1,
             act=1, d=1, bp=0):
        return lib.bevops_conv_slice_f16_ex(x, xp, w, b, r, rp, o, op, B, H, W, Cin, Cout, ks, s, act, d, bp, None)

    # (1) BAD_PARAM of the parent entry, and a dilation that is not positive
    assert call(H=0) == BAD_PARAM and call(B=-1) == BAD_PARAM and call(Cin=0) == BAD_PARAM and call(ks=0) == BAD_PARAM
    assert call(x=None) == BAD_PARAM and call(w=None) == BAD_PARAM and call(o=None) == BAD_PARAM
    assert call(x=p + 8) == BAD_PARAM and call(o=p + 770) == BAD_PARAM and call(b=p + 513) == BAD_PARAM
    assert call(xp=24) == BAD_PARAM and call(op=12) == BAD_PARAM and call(r=p + 1024, rp=12) == BAD_PARAM
    assert call(d=0) == BAD_PARAM and call(d=-6) == BAD_PARAM
    assert call(d=0, ks=5) == BAD_PARAM                                     # before the domain checks
    # (2) the per-image bias: below Cout, no multiple of 8, no bias, rows not 16-byte aligned
    assert call(bp=4) == BAD_PARAM and call(Cout=16, op=16, bp=8) == BAD_PARAM
    assert call(bp=12) == BAD_PARAM and call(bp=-8) == BAD_PARAM
    assert call(bp=8, b=None) == BAD_PARAM and call(bp=8, b=p + 512 + 2) == BAD_PARAM
    assert call(bp=12, ks=5) == BAD_PARAM and call(bp=4, d=2, s=2) == BAD_PARAM   # before the domain checks
    assert call(B=0, bp=4) == BAD_PARAM
    # (3) NOT_SUPPORTED of the parent entry
    assert call(Cin=48, xp=48) == NOT_SUPPORTED and call(Cout=12, op=16) == NOT_SUPPORTED
    assert call(ks=5) == NOT_SUPPORTED and call(s=3) == NOT_SUPPORTED and call(act=3) == NOT_SUPPORTED
    # (4) a dilation needs the 3 x 3 at stride 1
    assert call(d=2, ks=1) == NOT_SUPPORTED and call(d=6, s=2) == NOT_SUPPORTED and call(d=18, ks=1, s=2) == NOT_SUPPORTED
    assert call(B=0, d=1, ks=1) == SUCCESS and call(B=0, d=1, s=2) == SUCCESS
    # (5) the 32-bit byte offsets: the extent as in the parent entry, and the tap displacement with a dilation
    assert call(B=1, H=32768, W=2048, Cin=32) == NOT_SUPPORTED
    assert call(B=1, H=32768, W=1024, Cin=32, xp=64) == NOT_SUPPORTED
    assert call(B=0, H=2, W=1 << 20, xp=512, d=4) == NOT_SUPPORTED           # 4 * (2^20 + 1) * 512 * 2 > 2^31 - 1
    assert call(B=0, H=2, W=1 << 20, xp=512, d=1) == SUCCESS                 # (the parent's domain is unchanged)
    assert call(B=0, H=2, W=(1 << 19) - 2, xp=512, d=4) == SUCCESS
    # (6) nothing to do
    assert call(B=0) == SUCCESS and call(B=0, d=18) == SUCCESS and call(B=0, bp=8) == SUCCESS
    assert call(B=0, d=12, bp=16, b=p + 512, r=p + 1024, rp=16, xp=72, op=24) == SUCCESS


def test_parent_entry_keeps_its_statuses(lib, p):
    p = p[0]
    f = lib.bevops_conv_slice_f16
    assert f(p, 32, p + 256, p + 512, None, 0, p + 768, 8, 0, 4, 4, 32, 8, 3, 1, 2, None) == SUCCESS
    assert f(p, 32, p + 256, p + 514, None, 0, p + 768, 8, 0, 4, 4, 32, 8, 3, 1, 2, None) == SUCCESS   # a 2-byte aligned bias
    assert f(p, 32, p + 256, p + 512, None, 0, p + 768, 8, 1, 4, 4, 32, 8, 5, 1, 2, None) == NOT_SUPPORTED


def test_wrapper_checks_without_a_device():
    import torch

    import bevformer_tensorrt_amd as bev
    x = torch.zeros((1, 4, 4, 32), dtype=torch.float16).permute(0, 3, 1, 2)
    w = torch.zeros((8, 32, 3, 3), dtype=torch.float16)
    with pytest.raises(ValueError):                                           # not on the GPU: refused before any call
        bev.conv_slice_nhwc(x, w, dilation=6)
