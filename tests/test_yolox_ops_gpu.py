"""bevops_focus_nhwc, bevops_spp_maxpool_nhwc and bevops_upsample_nearest2x_nhwc (csrc/yolox.hip) through the C ABI in
the guarded arena of tests/util_arena.py, under both poisons.  All three are exact: copies and maxima."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util_exact_dense as X
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 8 << 20


def _lib():
    from bevformer_tensorrt_amd.utils import lib as L
    return L, L.load_library(), L.current_stream_ptr(torch.device("cuda"))


def _outside_untouched(before, after, c0, c1):
    mask = np.zeros(after.shape, bool)
    mask[..., c0:c1] = True
    assert np.array_equal(after.view(np.int16)[~mask], before.view(np.int16)[~mask]), "bytes outside the slice were written"


# ---------------------------------------------------------------------------------------------- Focus
@pytest.mark.parametrize("B,H,W", [(1, 2, 2), (1, 6, 10), (2, 34, 66)])
def test_focus_is_the_slicing_statement(B, H, W):
    L, h, st = _lib()
    r = X._rng("focus", B, H, W)
    img = r.standard_normal((B, 3, H, W)).astype(np.float16)
    t = torch.from_numpy(img)
    want = torch.cat((t[..., ::2, ::2], t[..., 1::2, ::2], t[..., ::2, 1::2], t[..., 1::2, 1::2]), dim=1)   # mmdet's Focus
    want = want.permute(0, 2, 3, 1).numpy()
    got = []
    for poison in POISONS:
        arena = Arena(CAPACITY, poison)
        imd = arena.place(t, 2, "image")
        pitch, c0 = 48, 8
        buf = arena.empty((B, H // 2, W // 2, pitch), torch.float16, 16, "out")
        before = buf.cpu().numpy().copy()
        assert h.bevops_focus_nhwc(imd.data_ptr(), buf[..., c0:].data_ptr(), pitch, B, H, W, st) == L.SUCCESS
        arena.check()
        after = buf.cpu().numpy()
        _outside_untouched(before, after, c0, c0 + 32)
        got.append(after[..., c0:c0 + 32].copy())
    assert np.array_equal(got[0].view(np.int16), got[1].view(np.int16))
    assert np.array_equal(got[0][..., :12].view(np.int16), want.view(np.int16))
    assert not got[0][..., 12:].view(np.int16).any(), "channels 12 .. 31 are zero"


# ---------------------------------------------------------------------------------------------- SPP
@pytest.mark.parametrize("C", [8, 40])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (5, 7), (13, 13), (20, 21)])
def test_spp_pools_inside_one_buffer(H, W, C):
    """x = slice 0 and out = slices 1 .. 3 of ONE [B, H, W, 4 C] buffer, against F.max_pool2d in float32; +-inf inputs;
    slice 0 keeps its bits."""
    L, h, st = _lib()
    B = 2
    r = X._rng("spp", H, W, C)
    x = r.standard_normal((B, H, W, C)).astype(np.float16)
    flat = x.reshape(-1)
    flat[r.integers(0, flat.size, size=max(1, flat.size // 50))] = np.inf
    flat[r.integers(0, flat.size, size=max(1, flat.size // 50))] = -np.inf
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).float()
    want = torch.cat([F.max_pool2d(xt, k, 1, k // 2) for k in (5, 9, 13)], dim=1).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(want.astype(np.float16).astype(np.float32), want)
    got = []
    for poison in POISONS:
        arena = Arena(CAPACITY, poison)
        buf = arena.empty((B, H, W, 4 * C), torch.float16, 16, "x|pools")
        buf[..., :C].copy_(torch.from_numpy(x))
        assert h.bevops_spp_maxpool_nhwc(buf.data_ptr(), 4 * C, buf[..., C:].data_ptr(), 4 * C, B, H, W, C, 5, 9, 13,
                                         st) == L.SUCCESS
        arena.check()
        after = buf.cpu().numpy()
        assert np.array_equal(after[..., :C].view(np.int16), x.view(np.int16)), "the input slice was written"
        got.append(after[..., C:].copy())
    assert np.array_equal(got[0].view(np.int16), got[1].view(np.int16))
    assert np.array_equal(got[0].view(np.int16), want.astype(np.float16).view(np.int16))


def test_spp_nan_reaches_every_window_that_holds_it():
    L, h, st = _lib()
    B, H, W, C = 1, 9, 9, 8
    x = np.zeros((B, H, W, C), np.float16)
    x[0, 4, 4, 3] = np.nan
    arena = Arena(CAPACITY, 0x55)
    xd = arena.place(torch.from_numpy(x), 16, "x")
    out = arena.empty((B, H, W, 3 * C), torch.float16, 16, "out")
    assert h.bevops_spp_maxpool_nhwc(xd.data_ptr(), C, out.data_ptr(), 3 * C, B, H, W, C, 5, 9, 13, st) == L.SUCCESS
    arena.check()
    got = np.isnan(out.cpu().numpy())
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for j, k in enumerate((5, 9, 13)):
        want = np.zeros((H, W, C), bool)
        want[..., 3] = np.maximum(np.abs(yy - 4), np.abs(xx - 4)) <= k // 2
        assert np.array_equal(got[0, ..., j * C:(j + 1) * C], want)


# ---------------------------------------------------------------------------------------------- up-sampling
@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (2, 3, 5, 40), (1, 20, 20, 16)])
def test_upsample_into_a_slice_at_an_offset(B, H, W, C):
    L, h, st = _lib()
    r = X._rng("upsample", B, H, W, C)
    x = r.standard_normal((B, H, W, C)).astype(np.float16)
    want = np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)
    ref = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2).float(), scale_factor=2, mode="nearest")
    assert np.array_equal(ref.permute(0, 2, 3, 1).numpy().astype(np.float16), want)
    got = []
    for poison in POISONS:
        arena = Arena(CAPACITY, poison)
        xp, xc0, op, oc0 = C + 8, 8, 2 * C + 16, C
        xbuf = arena.empty((B, H, W, xp), torch.float16, 16, "x")
        xbuf[..., xc0:].copy_(torch.from_numpy(x))
        obuf = arena.empty((B, 2 * H, 2 * W, op), torch.float16, 16, "out")
        before = obuf.cpu().numpy().copy()
        assert h.bevops_upsample_nearest2x_nhwc(xbuf[..., xc0:].data_ptr(), xp, obuf[..., oc0:].data_ptr(), op, B, H, W, C,
                                                st) == L.SUCCESS
        arena.check()
        after = obuf.cpu().numpy()
        _outside_untouched(before, after, oc0, oc0 + C)
        got.append(after[..., oc0:oc0 + C].copy())
    assert np.array_equal(got[0].view(np.int16), got[1].view(np.int16))
    assert np.array_equal(got[0].view(np.int16), want.view(np.int16))


# ---------------------------------------------------------------------------------------------- the Python side
def test_wrappers_write_slices_of_one_buffer():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.functions import yolox_ops as Y
    g = torch.Generator().manual_seed(3)
    img = torch.randn((2, 3, 12, 20), generator=g).half().cuda()
    f = bev.focus_nhwc(img)
    want = torch.cat((img[..., ::2, ::2], img[..., 1::2, ::2], img[..., ::2, 1::2], img[..., 1::2, 1::2]), dim=1)
    assert f.shape == (2, 32, 6, 10) and torch.equal(f[:, :12], want) and torch.count_nonzero(f[:, 12:]) == 0
    C = 16
    buf = Y.nhwc_empty(2, 4 * C, 6, 10, "cuda")
    buf[:, :C] = torch.randn((2, C, 6, 10), generator=g).half().cuda()
    x0 = buf[:, :C].clone()
    bev.spp_maxpool_nhwc(buf[:, :C], out=buf[:, C:])
    assert torch.equal(buf[:, :C], x0)
    for j, k in enumerate((5, 9, 13)):
        assert torch.equal(buf[:, (j + 1) * C:(j + 2) * C], F.max_pool2d(x0.float(), k, 1, k // 2).half())
    up = Y.nhwc_empty(2, 2 * C, 12, 20, "cuda")
    up.zero_()
    bev.upsample_nearest2x_nhwc(buf[:, C:2 * C], out=up[:, C:])
    assert torch.equal(up[:, C:], F.interpolate(buf[:, C:2 * C].float(), scale_factor=2, mode="nearest").half())
    assert torch.count_nonzero(up[:, :C]) == 0
    with pytest.raises(ValueError, match="channel slice"):
        bev.upsample_nearest2x_nhwc(torch.zeros((1, 8, 4, 4), device="cuda", dtype=torch.float16))   # planar, not channels-last
