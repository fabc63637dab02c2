"""bevops_centerpoint_decode_ex: a batch of maps that are channel slices of ONE packed channels-last tensor
[B, H, W, 32] (BEVDet's head output) read in place through (channel, pixel, item) strides.  The four outputs must be
bit-equal to the call on contiguous copies; pad channels and guard bands hold NaN, so a read outside a map shows."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SLICES = ((0, 2), (2, 3), (3, 6), (6, 8), (8, 10), (10, 20))       # reg, height, dim, rot, vel, heatmap
CODER = dict(max_num=60, post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], pc_range=[-51.2, -51.2],
             out_size_factor=8, voxel_size=[0.1, 0.1], score_threshold=0.1)
# 10 classes: 16 x 25 = 4 000 candidates (one launch), 10 x 41 = 4 100 (partial selection + final launch)
SIZES = [(16, 25), (10, 41)]


def _packed(B, H, W, seed):
    """[B, 32, H, W] view of a channels-last fp16 buffer with NaN guard bands around it and NaN in channels 20 .. 31"""
    g = torch.Generator().manual_seed(seed)
    guard = 4096
    flat = torch.full((guard + B * H * W * 32 + guard,), float("nan"), dtype=torch.float16)
    body = flat[guard:guard + B * H * W * 32].view(B, H, W, 32)
    body[..., :20] = torch.randn(B, H, W, 20, generator=g).half()
    body[..., 10:20] = (torch.randn(B, H, W, 10, generator=g) * 2 - 1).half()      # heat-map logits, some above 0.1
    flat = flat.cuda()
    return flat[guard:guard + B * H * W * 32].view(B, H, W, 32).permute(0, 3, 1, 2)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.fixture
def probe(monkeypatch):
    """records the map pointers each decode entry receives"""
    from bevformer_tensorrt_amd.utils import lib as L
    handle = L.load_library()
    calls = []
    for name in ("bevops_centerpoint_decode", "bevops_centerpoint_decode_ex"):
        real = getattr(handle, name)

        def wrapped(*args, _real=real, _name=name):
            calls.append((_name, tuple(args[1:7])))
            return _real(*args)
        monkeypatch.setattr(handle, name, wrapped)
    return calls


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("B", [1, 2, 3])
def test_slices_of_the_packed_tensor_are_read_in_place(B, H, W, probe):
    from bevformer_tensorrt_amd import functions as F
    packed = _packed(B, H, W, seed=B * 100 + H)
    maps = [packed[:, a:b] for a, b in SLICES]
    got = F.centerpoint_decode(*maps, padded=True, **CODER)
    name, ptrs = probe[-1]
    assert name == ("bevops_centerpoint_decode_ex" if B > 1 else "bevops_centerpoint_decode")
    assert list(ptrs) == [m.data_ptr() for m in maps]                 # no copy of a map
    want = F.centerpoint_decode(*[m.contiguous() for m in maps], padded=True, **CODER)
    assert probe[-1][0] == "bevops_centerpoint_decode"
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert _bits(a, b)
    boxes, scores, labels, count = got
    assert tuple(boxes.shape) == (B, 60, 9) and (count > 0).all() and not torch.isnan(boxes).any()
    # every batch item on its own equals its rows of the batched call
    for i in range(B):
        one = F.centerpoint_decode(*[m[i:i + 1].contiguous() for m in maps], padded=True, **CODER)
        for a, b in zip(got, one):
            assert _bits(a[i:i + 1], b)


@pytest.mark.parametrize("H,W", SIZES)
def test_dense_maps_keep_the_plain_entry_and_its_bits(H, W, probe):
    """Dense NCHW and dense channels-last maps (B = 2) go through bevops_centerpoint_decode as before; the _ex entry
    called with the dense item strides gives the same bits."""
    from bevformer_tensorrt_amd import functions as F
    from bevformer_tensorrt_amd.utils import lib as L
    B = 2
    packed = _packed(B, H, W, seed=7)
    nchw = [packed[:, a:b].contiguous() for a, b in SLICES]
    nhwc = [m.contiguous(memory_format=torch.channels_last) for m in nchw]
    a = F.centerpoint_decode(*nchw, padded=True, **CODER)
    b = F.centerpoint_decode(*nhwc, padded=True, **CODER)
    assert [c[0] for c in probe] == ["bevops_centerpoint_decode"] * 2
    for x, y in zip(a, b):
        assert _bits(x, y)
    handle = L.load_library()
    dev = packed.device
    chans = [hi - lo for lo, hi in SLICES]
    strides = (ctypes.c_int64 * 18)(*[v for c in chans for v in (H * W, 1, c * H * W)])
    out = (torch.empty(B, 60, 9, device=dev), torch.empty(B, 60, device=dev),
           torch.empty(B, 60, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    nws = handle.bevops_centerpoint_decode_workspace_size(B, 10, H, W, 60)
    ws = torch.empty(max(nws, 8), dtype=torch.uint8, device=dev)
    rng = (ctypes.c_float * 6)(*CODER["post_center_range"])
    st = handle.bevops_centerpoint_decode_ex(1, *[m.data_ptr() for m in nchw], strides, *[t.data_ptr() for t in out], B, 10,
                                             H, W, 60, 8.0, 0.1, 0.1, -51.2, -51.2, rng, 0.1, 1, 0, ws.data_ptr(), nws,
                                             L.current_stream_ptr(dev))
    assert st == 0
    torch.cuda.synchronize()
    for x, y in zip(a, out):
        assert _bits(x, y)
