"""CPU-only checks of BEVDet's `bev_half` switch: the merged operands (depth_net as a 128-column GEMM, the six heads
as a stacked and a block-diagonal convolution) against F.conv2d in float64, the default and its environment override,
the fall-back of "hip" to the torch statements off the GPU, the C ABI's argument checks and the wrappers' own."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util_bevpool import index_add_reference

SMALL_CFG = dict(grid_config=dict(x=[-6.4, 6.4, 0.8], y=[-6.4, 6.4, 0.8], z=[-5, 3, 8], depth=[1.0, 60.0, 1.0]),
                 input_size=(64, 176), downsample=16, in_channels=256, out_channels=64)


def test_depth_net_as_a_128_column_gemm():
    from bevformer_tensorrt_amd.bevdet import merge_depth_net
    g = torch.Generator().manual_seed(0)
    D, C, cin = 59, 64, 256
    w = torch.randn(D + C, cin, 1, 1, generator=g, dtype=torch.float64)
    b = torch.randn(D + C, generator=g, dtype=torch.float64)
    x = torch.randn(2, cin, 3, 5, generator=g, dtype=torch.float64)
    wm, bm, lay = merge_depth_net(w, b, D, C)
    assert lay == dict(row_stride=128, feat_offset=0, depth_offset=64)
    assert wm.shape == (128, cin) and bm.shape == (128,) and wm.dtype == torch.float64
    want = F.conv2d(x, w, b).permute(0, 2, 3, 1).reshape(-1, D + C)      # pixel rows: [depth 59 | features 64]
    rows = x.permute(0, 2, 3, 1).reshape(-1, cin)
    got = rows @ wm.t() + bm
    fo, do = lay["feat_offset"], lay["depth_offset"]
    assert fo % 8 == 0 and do % 8 == 0                                    # both ranges 16-byte aligned in fp16
    torch.testing.assert_close(got[:, fo:fo + C], want[:, D:], rtol=0, atol=1e-12)
    torch.testing.assert_close(got[:, do:do + D], want[:, :D], rtol=0, atol=1e-12)
    assert torch.equal(wm[do + D:], torch.zeros(128 - do - D, cin, dtype=torch.float64))
    assert torch.equal(got[:, do + D:], torch.zeros(rows.shape[0], 128 - do - D, dtype=torch.float64))
    # the rows are the source rows, moved: bit for bit
    assert torch.equal(wm[:C], w[D:, :, 0, 0]) and torch.equal(wm[do:do + D], w[:D, :, 0, 0])
    assert torch.equal(bm[:C], b[D:]) and torch.equal(bm[do:do + D], b[:D])
    with pytest.raises(ValueError):
        merge_depth_net(w, b, D + 1, C)
    # no bias: zero shift
    assert torch.equal(merge_depth_net(w, None, D, C)[1], torch.zeros(128, dtype=torch.float64))


def test_heads_as_a_stacked_and_a_block_diagonal_convolution():
    from bevformer_tensorrt_amd.bevdet import HEADS_R50, merge_heads
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    first = [(r(64, 64, 3, 3) * 0.05, r(64)) for _ in HEADS_R50]
    final = [(r(c, 64, 3, 3) * 0.05, r(c)) for _, c in HEADS_R50]
    s = r(1, 64, 9, 11)
    w1, b1, w2, b2, slices = merge_heads(first, final)
    assert w1.shape == (384, 64, 3, 3) and b1.shape == (384,) and w2.shape == (32, 384, 3, 3) and b2.shape == (32,)
    assert slices == [(0, 2), (2, 3), (3, 6), (6, 8), (8, 10), (10, 20)]
    got = F.conv2d(F.relu(F.conv2d(s, w1, b1, padding=1)), w2, b2, padding=1)
    for (wa, ba), (wb, bb), (lo, hi) in zip(first, final, slices):
        want = F.conv2d(F.relu(F.conv2d(s, wa, ba, padding=1)), wb, bb, padding=1)
        torch.testing.assert_close(got[:, lo:hi], want, rtol=0, atol=1e-10)
    assert torch.equal(got[:, 20:], torch.zeros(1, 12, 9, 11, dtype=torch.float64))
    # the layout itself: head i's final weights on input channels 64 i .. 64 i + 63, zero everywhere else
    mask = torch.zeros(32, 384, dtype=torch.bool)
    for i, (lo, hi) in enumerate(slices):
        mask[lo:hi, 64 * i:64 * (i + 1)] = True
        assert torch.equal(w2[lo:hi, 64 * i:64 * (i + 1)], final[i][0])
        assert torch.equal(w1[64 * i:64 * (i + 1)], first[i][0]) and torch.equal(b1[64 * i:64 * (i + 1)], first[i][1])
        assert torch.equal(b2[lo:hi], final[i][1])
    assert not w2[~mask].any() and not b2[20:].any()


def test_default_is_torch_and_the_environment_flips_it(monkeypatch):
    from bevformer_tensorrt_amd.bevdet import BEVDET_R50, BEVDet, LSSViewTransformer
    monkeypatch.delenv("BEVOPS_BEVDET_BEV_HALF", raising=False)
    m = BEVDet(cfg=SMALL_CFG)
    assert m.bev_half == "torch" and m.view.bev_half == "torch"
    assert LSSViewTransformer(**BEVDET_R50).bev_half == "torch"
    monkeypatch.setenv("BEVOPS_BEVDET_BEV_HALF", "hip")
    m = BEVDet(cfg=SMALL_CFG)
    assert m.bev_half == "hip" and m.view.bev_half == "hip"
    assert BEVDet(cfg=SMALL_CFG, bev_half="torch").bev_half == "torch"        # the argument wins over the environment
    monkeypatch.setenv("BEVOPS_BEVDET_BEV_HALF", "triton")
    with pytest.raises(ValueError):
        BEVDet(cfg=SMALL_CFG)
    with pytest.raises(ValueError):
        BEVDet(cfg=SMALL_CFG, bev_half="fast")


class _CpuOps:
    """An operator set that HAS the names the "hip" path looks for -- so what keeps the torch statements below is the
    tensors being fp32 on the CPU, not a missing function -- and pools with the oracle statement."""

    @staticmethod
    def bev_pool_v2_2(depth, feat, ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths, bev_h, bev_w):
        want = index_add_reference(depth.float().numpy(), feat.float().numpy(), ranks_depth.numpy(), ranks_feat.numpy(),
                                   ranks_bev.numpy(), bev_h, bev_w)
        return torch.from_numpy(want).to(depth.dtype)

    @staticmethod
    def _never(*a, **k):
        raise AssertionError("a HIP operator was reached from CPU / fp32 tensors")

    lss_depth_split = upsample_bilinear_concat_nhwc = conv_nhwc = conv3x3_auto = dense_auto = _never


def test_hip_on_a_cpu_fp32_model_runs_the_torch_statements():
    from bevformer_tensorrt_amd import bevdet as D
    a = D.BEVDet(cfg=SMALL_CFG, ops=_CpuOps, seed=0, bev_half="torch")
    b = D.BEVDet(cfg=SMALL_CFG, ops=_CpuOps, seed=0, bev_half="hip")
    b.load_state_dict(a.state_dict())
    ranks = a.view.get_bev_pool_input(*D.synthetic_rig(a.view))
    img = torch.randn(1, 6, 3, 64, 176, generator=torch.Generator().manual_seed(3))
    want, got = a(img, *ranks), b(img, *ranks)
    assert len(got) == 6
    for (name, c), x, y in zip(D.HEADS_R50, got, want):
        assert x.shape == y.shape == (1, c, 16, 16) and x.dtype == torch.float32, name
        assert torch.equal(x, y), name
    # prepare_bev_half itself works on the CPU (the merged operands live where the weights live)
    b.prepare_bev_half()
    assert b.view.depth_net_merged(build=False)[0].shape == (128, 256)
    assert b.heads_merged(build=False)[2].shape == (32, 384, 3, 3)
    # ... and follows the weights: a changed head weight makes the cached operand stale
    with torch.no_grad():
        b.heads["reg"][1].weight.add_(1.0)
    assert b.heads_merged(build=False) is None
    w2 = b.heads_merged()[2]
    assert torch.equal(w2[0:2, 0:64], b.heads["reg"][1].weight)


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def test_new_symbols_resolve(lib):
    from bevformer_tensorrt_amd.utils.lib import SIGNATURES
    import bevformer_tensorrt_amd.functions as fn
    for name in ("bevops_lss_depth_split", "bevops_upsample_bilinear_concat_nhwc"):
        assert name in SIGNATURES
        addr = lib.bevops_query(name.encode())
        assert addr and addr == ctypes.cast(getattr(lib, name), ctypes.c_void_p).value, name
    assert "lss_depth_split" in fn.__all__ and "upsample_bilinear_concat_nhwc" in fn.__all__
    from bevformer_tensorrt_amd.utils.register import TRT_FUNCTIONS
    assert "lss_depth_split" not in TRT_FUNCTIONS          # not one of the reference's registry functions


def test_abi_argument_checks_return_before_any_device_call(lib):
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    split, up = lib.bevops_lss_depth_split, lib.bevops_upsample_bilinear_concat_nhwc
    #          dtype x  depth feat n  hw  stride doff D  foff C
    assert split(0, p, p, p, 2, 15, 16, 8, 5, 0, 8, None) == 3            # fp32
    assert split(1, p, p, p, 2, 15, 512, 0, 257, 264, 8, None) == 3       # D = 257
    assert split(1, p, p, p, 2, 15, 512, 0, 0, 264, 8, None) == 3         # D = 0
    assert split(1, p, p, p, 2, 15, 32, 16, 5, 0, 12, None) == 2          # C = 12
    assert split(1, p, p, p, 2, 15, 32, 16, 5, 4, 8, None) == 2           # feat_offset = 4
    assert split(1, p, p, p, 2, 15, 16, 4, 5, 0, 8, None) == 2            # overlapping ranges
    assert split(1, p, p, p, 2, 15, 16, 12, 5, 0, 8, None) == 2           # depth columns leave the row
    assert split(1, p, p, p, 2, 15, 12, 8, 4, 0, 8, None) == 2            # row_stride = 12
    assert split(1, None, p, p, 2, 15, 16, 8, 5, 0, 8, None) == 2         # no input
    assert split(1, p + 2, p, p, 2, 15, 16, 8, 5, 0, 8, None) == 2        # misaligned rows
    assert split(1, p, p, p, 2, 0, 16, 8, 5, 0, 8, None) == 0             # hw = 0: success, no launch
    assert split(1, p, p, p, 0, 15, 16, 8, 5, 0, 8, None) == 0
    #       dtype a  b  out n  h  w  ca hb wb cb
    assert up(1, p, p, p, 1, 4, 4, 8, 2, 2, 12, None) == 2                # cb = 12
    assert up(1, p, p, p, 1, 4, 4, 12, 2, 2, 8, None) == 2                # ca = 12
    assert up(1, None, p, p, 1, 4, 4, 8, 2, 2, 8, None) == 2              # a == NULL with ca > 0
    assert up(0, p, p, p, 1, 4, 4, 8, 2, 2, 8, None) == 3                 # fp32
    assert up(1, p, p, p, 1, 0, 4, 8, 2, 2, 8, None) == 2                 # empty output
    assert up(1, p, p + 2, p, 1, 4, 4, 8, 2, 2, 8, None) == 2             # misaligned b


def test_wrapper_argument_checks():
    import bevformer_tensorrt_amd.functions as fn
    h = lambda *s: torch.zeros(*s, dtype=torch.float16)
    cl = lambda *s: h(*s).contiguous(memory_format=torch.channels_last)
    with pytest.raises(TypeError):
        fn.lss_depth_split(np.zeros((30, 16), np.float16), 2, 5, 8, 8)
    with pytest.raises(TypeError):
        fn.lss_depth_split(torch.zeros(30, 16), 2, 5, 8, 8)                # fp32
    with pytest.raises(TypeError, match="GPU"):
        fn.lss_depth_split(h(30, 16), 2, 5, 8, 8)                          # in the domain, but on the CPU
    for args in ((h(30, 16), 4, 5, 8, 8),            # 30 rows, 4 images
                 (h(30, 16), 2, 0, 8, 8), (h(30, 512), 2, 257, 8, 8),      # D outside 1 .. 256
                 (h(30, 32), 2, 5, 12, 16), (h(30, 32), 2, 5, 8, 16, 4),   # C = 12, feat_offset = 4
                 (h(30, 12), 2, 4, 8, 8),                                  # row_stride = 12
                 (h(30, 16), 2, 5, 8, 4), (h(30, 16), 2, 5, 8, 12),        # overlap, depth leaves the row
                 (h(30, 2, 8), 2, 5, 8, 8), (h(30, 32)[:, :16], 2, 5, 8, 8)):   # not 2-D, not contiguous
        with pytest.raises(ValueError):
            fn.lss_depth_split(*args)
    with pytest.raises(ValueError):
        fn.lss_depth_split(h(30, 16), 2, 5, 8, 8, spatial=(4, 4))
    up = fn.upsample_bilinear_concat_nhwc
    with pytest.raises(TypeError):
        up(None, torch.zeros(1, 8, 2, 2), scale_factor=2)
    with pytest.raises(TypeError):
        up(torch.zeros(1, 8, 4, 4), cl(1, 8, 2, 2))
    with pytest.raises(TypeError, match="GPU"):
        up(cl(1, 8, 4, 4), cl(1, 8, 2, 2))
    for a, b, kw in ((None, cl(1, 12, 2, 2), dict(scale_factor=2)), (cl(1, 12, 4, 4), cl(1, 8, 2, 2), {}),
                     (None, cl(1, 8, 2, 2), {}), (None, cl(1, 8, 2, 2), dict(scale_factor=1.5)),
                     (None, h(1, 8, 2, 2), dict(scale_factor=2)),          # NCHW
                     (cl(2, 8, 4, 4), cl(1, 8, 2, 2), {}), (cl(1, 8, 4, 4), cl(1, 8, 2, 2), dict(size=(5, 5))),
                     (None, cl(1, 8, 2, 2), dict(size=(0, 4)))):
        with pytest.raises(ValueError):
            up(a, b, **kw)


def test_decode_reads_a_channel_slice_in_place_for_one_batch_item():
    """functions.decode._map_strides: a [1, c, H, W] channel slice of a wider channels-last tensor is passed as it is,
    with channel stride 1 and the packed tensor's channel count as the pixel stride; B > 1 keeps the copy; contiguous
    and channels-last inputs are handled as before."""
    from bevformer_tensorrt_amd.functions.decode import _map_strides
    packed = torch.arange(16 * 16 * 32, dtype=torch.float32).view(1, 16, 16, 32).permute(0, 3, 1, 2)
    for lo, hi in ((0, 2), (2, 3), (3, 6), (10, 20)):
        s = packed[:, lo:hi]
        t, cs, ps = _map_strides(s, "x")
        assert t is s and (cs, ps) == (1, 32), (lo, hi)
    two = torch.zeros(2, 16, 16, 32).permute(0, 3, 1, 2)[:, 3:6]
    t, cs, ps = _map_strides(two, "x")
    assert t is not two and t.is_contiguous() and (cs, ps) == (256, 1)
    c = torch.zeros(1, 3, 16, 16)
    assert _map_strides(c, "x") == (c, 256, 1)
    cl = c.contiguous(memory_format=torch.channels_last)
    t, cs, ps = _map_strides(cl, "x")
    assert t is cl and (cs, ps) == (1, 3)
    odd = torch.zeros(1, 16, 32, 16).permute(0, 2, 1, 3)[:, 3:6]        # a slice whose pixels are not row-major: copy
    t, cs, ps = _map_strides(odd, "x")
    assert t is not odd and (cs, ps) == (256, 1)
