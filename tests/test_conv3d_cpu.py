"""bevops_conv3d_slice_f16 / functions.conv3d without a GPU: the entry's statuses in their documented order on dummy
pointers (every one returns before a device call), the taps repack, the plain-path statement and the public names."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

BAD, UNSUPPORTED = 2, 3
# x_pitch, res_pitch, out_pitch, B, Z, Y, X, Cin, Cout, ksize, stride, act
GOOD = dict(xp=32, rp=32, op=32, B=0, Z=4, Y=4, X=4, Cin=32, Cout=32, k=3, s=1, act=1)


def _entry(ptrs=(), **kw):
    from bevformer_tensorrt_amd.utils import load_library
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    a = dict(GOOD, x=p, w=p, bias=p, res=p, out=p)
    a.update(kw)
    a.update({name: p + 8 for name in ptrs})           # 8-byte aligned only
    return load_library().bevops_conv3d_slice_f16(a["x"], a["xp"], a["w"], a["bias"], a["res"], a["rp"], a["out"], a["op"],
                                                  a["B"], a["Z"], a["Y"], a["X"], a["Cin"], a["Cout"], a["k"], a["s"],
                                                  a["act"], None)


# every BAD_PARAM case also carries a NOT_SUPPORTED defect (ksize 5): the BAD_PARAM checks stand in front
@pytest.mark.parametrize("kw", [dict(x=None), dict(w=None), dict(out=None), dict(Z=0), dict(Y=-1), dict(X=0), dict(Cin=0),
                                dict(Cout=0), dict(B=-1), dict(xp=24), dict(op=24), dict(rp=24), dict(xp=36), dict(op=36),
                                dict(rp=36), dict(ptrs=("x",)), dict(ptrs=("w",)), dict(ptrs=("res",)),
                                dict(ptrs=("bias",)), dict(ptrs=("out",))], ids=str)
def test_bad_param(kw):
    assert _entry(**dict(kw, k=5)) == BAD
    assert _entry(**kw) == BAD


@pytest.mark.parametrize("kw", [dict(Cin=48, xp=48), dict(Cout=36, op=40, rp=40), dict(k=2), dict(k=5), dict(s=3), dict(s=0),
                                dict(act=2), dict(act=-1),
                                dict(B=1, Z=4096, Y=4096, X=8),                    # 2^27 voxels of 64 bytes: 2^33 bytes
                                dict(B=0x7fffffff, Z=0x7fffffff, Y=0x7fffffff, X=0x7fffffff),   # the product passes 2^64
                                dict(Cin=1 << 20, xp=1 << 20, Cout=1 << 10, op=1 << 10, rp=1 << 10),  # 27 * 2^31 weight bytes
                                dict(B=0, Z=1, Y=1 << 13, X=1 << 13, xp=32)],      # tap displacement 2^26 voxels * 64 bytes
                         ids=str)
def test_not_supported(kw):
    assert _entry(**kw) == UNSUPPORTED


def test_last_sizes_inside_the_limits_and_empty_batch():
    assert _entry() == 0 and _entry(bias=None, res=None, rp=0) == 0               # B == 0: success, nothing launched
    # (Y X + X + 1) x_pitch 2 = 0x7FFFFFC0 <= 0x7FFFFFFF with x_pitch 32: Y X + X + 1 = 2^25 - 1
    assert _entry(Z=1, Y=(1 << 12) - 1, X=1 << 13, xp=32) == UNSUPPORTED           # 2^25 + 1
    assert _entry(Z=1, Y=(1 << 12) - 2, X=(1 << 13) + 1, xp=32) == 0               # 4094 * 8193 + 8193 + 1 < 2^25


def test_taps_repack_indexing():
    from bevformer_tensorrt_amd.functions import conv3d_taps_weight
    w = torch.arange(8 * 32 * 27, dtype=torch.float32).view(8, 32, 3, 3, 3)
    taps = conv3d_taps_weight(w)
    assert tuple(taps.shape) == (8, 3, 3, 3, 32) and taps.is_contiguous() and conv3d_taps_weight(w) is taps
    for co, ci, kz, ky, kx in ((0, 0, 0, 0, 0), (7, 31, 2, 2, 2), (3, 5, 0, 1, 2), (4, 17, 2, 0, 1)):
        assert taps[co, kz, ky, kx, ci] == w[co, ci, kz, ky, kx]
    w.add_(1)                                                                       # a changed weight is repacked
    assert conv3d_taps_weight(w, build=False) is None and conv3d_taps_weight(w)[7, 2, 2, 2, 31] == w[7, 31, 2, 2, 2]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", [1, 3])
def test_plain_path_statement(stride, k):
    """CPU tensors take the torch statement: relu(conv + bias + identity), the identity in front of the activation."""
    from bevformer_tensorrt_amd.functions import conv3d_ndhwc, conv3d_taps
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 32, 5, 4, 7, generator=g, dtype=torch.float64)
    w = torch.randn(8, 32, k, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(8, generator=g, dtype=torch.float64) - 3
    conv = F.conv3d(x, w, b, stride, k // 2)
    res = torch.rand(conv.shape, generator=g, dtype=torch.float64) * 4
    want = F.relu(conv + res)
    assert (want != F.relu(conv) + res).float().mean() > 0.25                      # the order matters on these operands
    got = conv3d_ndhwc(x, w, b, "relu", res, stride)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    out = torch.empty_like(want)
    assert conv3d_taps(x, w.permute(0, 2, 3, 4, 1).contiguous(), b, "relu", res, stride, out=out) is out
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(conv3d_ndhwc(x, w, None, "none", None, stride), F.conv3d(x, w, None, stride, k // 2), atol=1e-12)


def test_public_names():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd import functions as fn
    for name in ("conv3d_ndhwc", "conv3d_taps"):
        assert name in fn.__all__ and getattr(bev, name) is getattr(fn, name) and name not in bev.TRT_FUNCTIONS
    assert fn.conv3d_ndhwc.__module__ == "bevformer_tensorrt_amd.functions.conv3d"
    from bevformer_tensorrt_amd.bevdet import BEVDET_OCC_R50
    assert BEVDET_OCC_R50["bev_encoder"] == "3d" and BEVDET_OCC_R50["occ_head"] == dict(Dz=16, num_classes=18, hidden=64)
