"""The int8 data-movement layers of csrc/yolox.hip (bevops_focus_nhwc_q, bevops_spp_maxpool_nhwc_s8,
bevops_upsample_nearest2x_nhwc_s8) in the guarded arena of tests/util_arena.py, under both poisons: every byte compared
exactly with a numpy statement, the bytes of the output buffer outside the output slice included."""
import numpy as np
import pytest
import torch

from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 8 << 20


def _lib():
    from bevformer_tensorrt_amd.utils import lib as L
    return L, L.load_library(), L.current_stream_ptr(torch.device("cuda"))


def _outside_unchanged(before, after, c0, C):
    mask = np.zeros(after.shape, bool)
    mask[..., c0:c0 + C] = True
    assert np.array_equal(after[~mask], before[~mask]), "bytes outside the output slice were written"


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("B,H,W,pitch,c0", [(1, 2, 2, 32, 0), (2, 6, 10, 64, 16), (1, 14, 18, 48, 16)])
def test_focus_q_ties_and_saturation(B, H, W, pitch, c0, poison):
    """The image on the tie grid (k + t) * scale, t in {0, +-1/4, +-1/2}, |k| up to 300: exact ties (rne: 2.5 -> 2,
    -3.5 -> -4) and saturation at +-127; scale 2^-5, so x * (1 / scale) is exact in fp32."""
    L, h, st = _lib()
    r = np.random.default_rng(B * 1000 + H)
    scale = 2.0 ** -5
    k = np.where(r.random((B, 3, H, W)) < 0.15, r.integers(-300, 301, (B, 3, H, W)), r.integers(-130, 131, (B, 3, H, W)))
    img = ((k + r.choice(np.array([0.0, 0.25, -0.25, 0.5, -0.5]), size=k.shape)) * scale)
    img.reshape(-1)[:4] = np.array([2.5, -3.5, 300.5, -300.5]) * scale
    img16 = img.astype(np.float16)
    assert np.array_equal(img16.astype(np.float64), img)
    q = np.clip(np.rint(img / scale), -127, 127).astype(np.int8)
    assert (q == 127).any() and (q == -127).any() and (np.abs(img / scale % 1.0) == 0.5).any()
    tl, tr, bl, br = q[..., ::2, ::2], q[..., ::2, 1::2], q[..., 1::2, ::2], q[..., 1::2, 1::2]
    want = np.zeros((B, H // 2, W // 2, 32), np.int8)
    want[..., :12] = np.concatenate((tl, bl, tr, br), axis=1).transpose(0, 2, 3, 1)
    arena = Arena(CAPACITY, poison)
    imgd = arena.place(torch.from_numpy(img16), 2, "image")
    obuf = arena.empty((B, H // 2, W // 2, pitch), torch.int8, 16, "out")
    before = obuf.cpu().numpy().copy()
    ov = obuf[..., c0:c0 + 32]
    assert h.bevops_focus_nhwc_q(imgd.data_ptr(), scale, ov.data_ptr(), pitch, B, H, W, st) == L.SUCCESS
    arena.check()
    after = obuf.cpu().numpy()
    _outside_unchanged(before, after, c0, 32)
    assert np.array_equal(after[..., c0:c0 + 32], want)


def _pool(x, k):
    """max over the k x k window, -128 outside the map: x [B, H, W, C] int8"""
    r = k // 2
    B, H, W, C = x.shape
    p = np.full((B, H + 2 * r, W + 2 * r, C), -128, np.int8)
    p[:, r:r + H, r:r + W] = x
    out = np.full_like(x, -128)
    for dy in range(k):
        for dx in range(k):
            out = np.maximum(out, p[:, dy:dy + H, dx:dx + W])
    return out


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("C", [16, 48])
@pytest.mark.parametrize("B,H,W", [(2, 3, 4), (1, 13, 13)])
def test_spp_pools_on_slices_of_one_buffer(B, H, W, C, poison):
    """x = slice 0 and out = slices 1 .. 3 of ONE [B, H, W, 4 C + 16] buffer; maps smaller than the windows (3 x 4) and
    13 x 13; the input holds -128 and 127."""
    L, h, st = _lib()
    r = np.random.default_rng(H * 100 + C)
    x = r.integers(-128, 128, (B, H, W, C)).astype(np.int8)
    x.reshape(-1)[:2] = (-128, 127)
    x[:, H // 2, W // 2, :8] = -128                      # a centre of -128: a window always holds its centre
    pitch = 4 * C + 16
    arena = Arena(CAPACITY, poison)
    buf = arena.empty((B, H, W, pitch), torch.int8, 16, "x|out")
    buf[..., :C].copy_(torch.from_numpy(x))
    before = buf.cpu().numpy().copy()
    assert h.bevops_spp_maxpool_nhwc_s8(buf.data_ptr(), pitch, buf[..., C:].data_ptr(), pitch, B, H, W, C, 5, 9, 13,
                                        st) == L.SUCCESS
    arena.check()
    after = buf.cpu().numpy()
    _outside_unchanged(before, after, C, 3 * C)
    for j, k in enumerate((5, 9, 13)):
        assert np.array_equal(after[..., (j + 1) * C:(j + 2) * C], _pool(x, k)), k
    if (H, W) == (3, 4):
        assert (after[..., 3 * C:4 * C] == x.max(axis=(1, 2), keepdims=True)).all()       # 13 x 13 covers the 3 x 4 map


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("C", [16, 48])
def test_upsample_is_a_byte_copy(C, poison):
    L, h, st = _lib()
    B, H, W = 2, 3, 5
    x = np.random.default_rng(C).integers(-128, 128, (B, H, W, C)).astype(np.int8)
    arena = Arena(CAPACITY, poison)
    xbuf = arena.empty((B, H, W, C + 16), torch.int8, 16, "x")
    xbuf[..., 16:].copy_(torch.from_numpy(x))
    obuf = arena.empty((B, 2 * H, 2 * W, 2 * C + 32), torch.int8, 16, "out")
    before = obuf.cpu().numpy().copy()
    assert h.bevops_upsample_nearest2x_nhwc_s8(xbuf[..., 16:].data_ptr(), C + 16, obuf[..., C:].data_ptr(), 2 * C + 32, B, H,
                                               W, C, st) == L.SUCCESS
    arena.check()
    after = obuf.cpu().numpy()
    _outside_unchanged(before, after, C, C)
    assert np.array_equal(after[..., C:2 * C], x.repeat(2, axis=1).repeat(2, axis=2))


def test_python_layer_routes_by_dtype():
    """spp_maxpool_nhwc / upsample_nearest2x_nhwc on int8 slices reach the int8 entries (the fp16 entries would refuse
    C = 16 pitches or read halves), allocate int8 results, and equal the numpy statement; focus_nhwc_q allocates."""
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.functions.yolox_ops import nhwc_empty
    dev = torch.device("cuda")
    x = torch.randint(-128, 128, (2, 5, 6, 16), dtype=torch.int8)
    buf = nhwc_empty(2, 64, 5, 6, dev, torch.int8)
    buf[:, :16].copy_(x.permute(0, 3, 1, 2))
    out = bev.spp_maxpool_nhwc(buf[:, :16], out=buf[:, 16:])
    assert out.dtype == torch.int8 and np.array_equal(buf[:, 48:].permute(0, 2, 3, 1).cpu().numpy(), _pool(x.numpy(), 13))
    fresh = bev.spp_maxpool_nhwc(buf[:, :16])
    assert fresh.dtype == torch.int8 and torch.equal(fresh, buf[:, 16:])
    up = bev.upsample_nearest2x_nhwc(buf[:, :16])
    assert up.dtype == torch.int8 and tuple(up.shape) == (2, 16, 10, 12)
    assert np.array_equal(up.permute(0, 2, 3, 1).cpu().numpy(), x.numpy().repeat(2, axis=1).repeat(2, axis=2))
    img = torch.randn((1, 3, 8, 8), device=dev).half()
    f = bev.focus_nhwc_q(img, 0.03)
    assert f.dtype == torch.int8 and tuple(f.shape) == (1, 32, 4, 4) and not f[:, 12:].any() and f[:, :12].any()
    with pytest.raises(ValueError, match="positive finite scale"):
        bev.focus_nhwc_q(img, 0.0)
