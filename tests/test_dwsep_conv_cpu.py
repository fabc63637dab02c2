"""CPU-only: the status contract of bevops_dwsep_conv_f16 (csrc/dwsep_conv.hip) in its documented order, the weight pack
of functions/yolox_ops.dwsep_conv_packed_weight against the stated layout and BN fold, and the refusals."""
import ctypes

import pytest
import torch

SUCCESS, BAD_PARAM, NOT_SUPPORTED = 0, 2, 3


def test_status_codes_in_their_order_without_gpu():
    import bevformer_tensorrt_amd as bev
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.utils import load_library
    lib = load_library()
    assert lib.bevops_query(b"bevops_dwsep_conv_f16") == ctypes.cast(lib.bevops_dwsep_conv_f16, ctypes.c_void_p).value
    for name in ("dwsep_conv_nhwc", "dwsep_conv_taps", "dwsep_conv_packed_weight"):
        assert name in fn.__all__ and getattr(bev, name) is getattr(fn, name) and name not in bev.TRT_FUNCTIONS
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 255) & ~255             # aligned host address: never dereferenced

    def call(x=p, xp=32, wd=p + 256, bd=p + 512, wp=p + 768, bp=p + 1024, r=None, rp=0, o=p + 1280, op=8, B=1, H=4, W=4,
             Cin=32, Cout=8, s=1, ad=2, ap=2):
        return lib.bevops_dwsep_conv_f16(x, xp, wd, bd, wp, bp, r, rp, o, op, B, H, W, Cin, Cout, s, ad, ap, None)

    r = p + 2048
    bad = [dict(x=None), dict(wd=None), dict(wp=None), dict(o=None), dict(B=-1), dict(H=0), dict(W=-1), dict(Cin=0),
           dict(Cout=0), dict(s=0), dict(xp=24), dict(op=0), dict(r=r, rp=0), dict(xp=36), dict(op=12), dict(r=r, rp=12),
           dict(x=p + 8), dict(wd=p + 264), dict(bd=p + 520), dict(wp=p + 776), dict(bp=p + 1025), dict(o=p + 1282),
           dict(r=r + 8, rp=8), dict(Cin=48, xp=40), dict(s=3, x=p + 8)]           # (the last two: before the domain)
    unsupported = [dict(Cin=48, xp=48), dict(Cout=12, op=16), dict(s=3), dict(ad=3), dict(ap=-1), dict(H=32768, W=2048),
                   dict(H=32768, W=1024, xp=64), dict(B=0, Cin=48, xp=48)]         # (the last: before B == 0)
    assert [kw for kw in bad if call(**kw) != BAD_PARAM] == []
    assert [kw for kw in unsupported if call(**kw) != NOT_SUPPORTED] == []
    assert call(B=0) == SUCCESS and call(B=0, bd=None, bp=None, r=r, rp=16) == SUCCESS


def test_pack_is_the_stated_layout_of_the_folded_weights():
    from bevformer_tensorrt_amd.checkpoint import fold_conv_bn
    from bevformer_tensorrt_amd.functions.yolox_ops import dwsep_conv_packed_weight as pack
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)                              # noqa: E731
    C, Co, eps = 16, 24, 1e-3
    wd, wp, gamma, beta, mean, var = r(C, 1, 3, 3), r(Co, C, 1, 1), r(C), r(C), r(C), r(C).abs() + 0.5
    fw, fb = fold_conv_bn(wd, None, gamma, beta, mean, var, eps)
    scale = gamma / torch.sqrt(var + eps)                     # the fold restated
    assert torch.allclose(fw, wd * scale[:, None, None, None], rtol=0, atol=1e-12)
    assert torch.allclose(fb, beta - mean * scale, rtol=0, atol=1e-12)
    taps, pw = pack(fw, wp)                                   # default widths: the next multiple of 32
    assert taps.shape == (3, 3, 32) and pw.shape == (32, 32) and taps.is_contiguous() and pw.is_contiguous()
    assert all(torch.equal(taps[ky, kx, :C], fw[:, 0, ky, kx]) for ky in range(3) for kx in range(3))
    assert torch.equal(pw[:Co, :C], wp[:, :, 0, 0]) and not taps[:, :, C:].any() and not pw[Co:].any() and not pw[:, C:].any()
    assert pack(fw, wp)[0] is taps and pack(fw, wp, build=False)[1] is pw and pack(fw, wp, 64, 32, build=False) is None
    wp.mul_(2.0)                                              # a changed weight is stale, then repacked
    assert pack(fw, wp, build=False) is None and torch.equal(pack(fw, wp)[1], 2.0 * pw)
    with pytest.raises(ValueError):
        pack(fw, wp, 8, 32)


def test_wrapper_and_model_refusals():
    from bevformer_tensorrt_amd.functions import dwsep_conv_taps
    from bevformer_tensorrt_amd.quantization import build_int8_yolox
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_NANO, YOLOX_S, DWSepConvAct
    with pytest.raises(ValueError, match="fp16 CUDA"):
        dwsep_conv_taps(torch.zeros((1, 32, 4, 4)).half(), torch.zeros(3, 3, 32).half(), None, torch.zeros(8, 32).half(), None)
    nano = YOLOX(YOLOX_NANO)      # stage heads, bottlenecks, down-samples, PAFPN bottlenecks, towers
    assert sum(isinstance(m, DWSepConvAct) for m in nano.modules()) == 4 + 8 + 2 + 4 + 12
    assert not any(isinstance(m, DWSepConvAct) for m in YOLOX(YOLOX_S).modules())
    with pytest.raises(NotImplementedError, match="use_depthwise"):
        build_int8_yolox(nano, "cpu", iter(()))               # before any frame runs
