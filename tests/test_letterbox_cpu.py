"""CPU-only checks of the 2-D detectors' camera front end (design/letterbox.md): the host geometry of the two test
pipelines against a hand-checked table; properties of the numpy restatement (tests/util_letterbox.py) that do not depend
on it -- the fixed-point flavour against float64 bilinear interpolation and against PIL, the float flavour against
float64, the observable normalise-after order; the status codes of bevops_image_letterbox and the exports."""
import ctypes

import numpy as np
import pytest
import torch

import util_letterbox as U

# (H0, W0), detector, resized, offset, canvas before the square padding, padded, border
GEOMETRY = [
    ((480, 640), "yolox", (480, 640), (0, 0), None, (640, 640), None),
    ((900, 1600), "yolox", (360, 640), (0, 0), None, (640, 640), None),
    ((1080, 1920), "yolox", (360, 640), (0, 0), None, (640, 640), None),
    ((480, 640), "centernet", (480, 640), (16, 16), (512, 672), (672, 672), [16, 496, 16, 656]),
    ((427, 640), "centernet", (427, 640), (11, 16), (448, 672), (672, 672), [11, 438, 16, 656]),
    ((900, 1600), "centernet", (360, 640), (12, 16), (384, 672), (672, 672), [12, 372, 16, 656]),
]

# (H0, W0) -> (Hs, Ws) of the fixed-point / float properties: identity, both up-scales with every clamp, odd rows, the
# area form, 2 : 1 in one axis only, a strong reduction, integer taps
RESIZES = [((1, 1), (1, 1)), ((2, 3), (5, 7)), ((45, 70), (36, 56)), ((37, 53), (64, 92)), ((64, 64), (32, 32)),
           ((64, 66), (32, 32)), ((100, 141), (29, 41)), ((108, 192), (36, 64)), ((20, 24), (30, 36)), ((7, 5), (7, 5))]


def planes(seed, H, W, kind="noise"):
    """[3, H, W] uint8: noise, a 0 / 255 checkerboard, or a constant."""
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (3, H, W), dtype=np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:H, 0:W]
        return np.broadcast_to((((yy + xx) & 1) * 255).astype(np.uint8), (3, H, W)).copy()
    return np.full((3, H, W), seed, np.uint8)


@pytest.mark.parametrize("src,det,size,offset,crop,canvas,border", GEOMETRY)
def test_geometry_table(src, det, size, offset, crop, canvas, border):
    import bevformer_tensorrt_amd as bev
    assert bev.keep_ratio_size(*src, (640, 640)) == size == U.keep_ratio_size(*src)
    g = (bev.yolox_test_geometry if det == "yolox" else bev.centernet_test_geometry)(*src)
    assert g["size"] == size and g["offset"] == offset
    assert g["img_shape"] == size + (3,) and g["pad_shape"] == canvas + (3,) and g["batch_input_shape"] == canvas
    sf = g["scale_factor"]
    assert sf.dtype == np.float32 and sf.shape == (4,)
    want = np.array([size[1] / src[1], size[0] / src[0]] * 2, dtype=np.float32)
    assert np.array_equal(sf, want)
    if det == "centernet":
        assert g["crop_shape"] == crop
        assert g["border"].dtype == np.float32 and g["border"].tolist() == border
    else:
        assert "border" not in g


def test_geometry_scale_factors_and_metas():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import _meta_rows
    assert np.array_equal(bev.yolox_test_geometry(480, 640)["scale_factor"], np.ones(4, np.float32))
    assert np.array_equal(bev.yolox_test_geometry(900, 1600)["scale_factor"], np.full(4, np.float32(0.4)))
    g = bev.centernet_test_geometry(96, 128, img_scale=(128, 128))
    assert g["size"] == (96, 128) and g["offset"] == (16, 16) and g["pad_shape"] == (160, 160, 3)
    assert g["border"].tolist() == [16, 112, 16, 144]
    # the dicts are img_metas entries as the host decoders read them
    assert _meta_rows([g], "border", (2, 0)) == [[16.0, 16.0]] and _meta_rows([g], "scale_factor") == [[1.0] * 4]
    p = bev.DETECT2D_IMAGE_PIPELINES
    assert p["yolox"]["arith"] == 0 and p["yolox"]["pad"] == [114.0] * 3 and not p["yolox"]["to_rgb"]
    assert p["centernet"]["arith"] == 1 and p["centernet"]["pad"] == [0.0] * 3 and p["centernet"]["to_rgb"]
    for name in ("yolox", "centernet"):
        assert p[name]["img_scale"] == (640, 640)
        for k in ("arith", "mean", "std", "to_rgb", "pad"):
            assert list(np.atleast_1d(p[name][k])) == list(np.atleast_1d(U.PIPELINES[name][k])), (name, k)


def test_get_bboxes_accept_the_geometry_dicts_as_img_metas():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import centernet_get_bboxes, yolox_get_bboxes
    g = torch.Generator().manual_seed(3)
    geo = bev.centernet_test_geometry(96, 128, img_scale=(128, 128))               # a 160 x 160 input, stride 4
    heat, wh, off = torch.rand(1, 5, 40, 40, generator=g), torch.rand(1, 2, 40, 40, generator=g) * 20, torch.rand(1, 2, 40, 40, generator=g)
    boxes, labels = centernet_get_bboxes(heat, wh, off, [geo], topk=10)[0]
    plain, _ = centernet_get_bboxes(heat, wh, off, [dict(batch_input_shape=(160, 160))], rescale=False, topk=10)[0]
    assert boxes.shape == (10, 5) and labels.shape == (10,)
    assert torch.allclose(boxes[:, :4], plain[:, :4] - 16.0, atol=1e-4)            # border (16, 16), scale_factor 1
    geo = bev.yolox_test_geometry(45, 60, img_scale=(96, 96))                      # 72 x 96 in a 96 x 96 input, scale 1.6
    assert geo["size"] == (72, 96) and geo["pad_shape"] == (96, 96, 3)
    maps = lambda c: [torch.randn(1, c, 96 // s, 96 // s, generator=g) for s in (8, 16, 32)]
    cls, reg, obj = maps(3), maps(4), maps(1)
    scaled, _ = yolox_get_bboxes(cls, reg, obj, [geo], score_thr=0.0, iou_threshold=1.0)[0]
    plain, _ = yolox_get_bboxes(cls, reg, obj, [geo], rescale=False, score_thr=0.0, iou_threshold=1.0)[0]
    assert scaled.shape == plain.shape and scaled.shape[0] > 0
    assert torch.allclose(scaled[:, :4], plain[:, :4] / torch.from_numpy(geo["scale_factor"]), rtol=1e-5)


# --------------------------------------------------------------------------- the fixed-point flavour
def test_fixed_bound_is_the_derived_one():
    assert U.FIXED_BOUND == 2 * 255 * 2.0 ** -11 * (1 + 2.0 ** -11) + 2.0 ** -7 + 0.5 + 0.5
    assert 1.25 < U.FIXED_BOUND < 1.26


@pytest.mark.parametrize("src,size", RESIZES)
def test_fixed_point_properties(src, size):
    worst = 0.0
    for kind, seed in (("noise", 3), ("checker", 0), ("const", 0), ("const", 255), ("const", 114)):
        x = planes(seed, *src, kind=kind)
        r = U.resize_u8(x, *size, clip=False)
        assert r.shape == (3,) + size and r.min() >= 0 and r.max() <= 255                   # before the uint8 cast
        assert np.array_equal(U.resize_u8(x, *size), r.astype(np.uint8))
        if kind == "const":
            assert (r == seed).all()                                                        # constants stay constant
        if src == size:
            assert np.array_equal(r, x)                                                     # identity at scale 1
        err = np.abs(r - U.bilinear_f64(x, *size)).max()
        worst = max(worst, float(err))
        assert err <= U.FIXED_BOUND, (kind, err)
    print(f"fixed point {src} -> {size}: largest distance from float64 bilinear {worst:.4f} (bound {U.FIXED_BOUND:.4f})")


@pytest.mark.parametrize("src,size", [(s, d) for s, d in RESIZES if d[0] >= s[0] and d[1] >= s[1]])
def test_fixed_point_against_pil_on_upscales(src, size):
    """For out >= in Pillow's BILINEAR triangle filter is the same interpolation (its own 8-bit arithmetic)."""
    from PIL import Image
    for kind, seed in (("noise", 5), ("checker", 0)):
        x = planes(seed, *src, kind=kind)
        pil = np.asarray(Image.fromarray(np.ascontiguousarray(x.transpose(1, 2, 0))).resize(size[::-1], Image.BILINEAR))
        diff = np.abs(U.resize_u8(x, *size).astype(np.int32) - pil.transpose(2, 0, 1).astype(np.int32)).max()
        print(f"fixed point {src} -> {size} ({kind}): largest difference from PIL {diff}")
        assert diff <= U.FIXED_BOUND + 0.5


def test_area_form_exactly_when_both_axes_are_two_to_one():
    x = planes(9, 64, 64)
    s = x.astype(np.int32)
    area = (s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2] + 2) >> 2
    assert np.array_equal(U.resize_u8(x, 32, 32), area.astype(np.uint8))
    # (on uint8 sources the general form with every weight 1024 / 0.5 gives the same values -- (1024 * 64 (a + b)) >> 16
    # and the float32 sums of integers are exact -- so the switch itself is pinned by the geometry rule below)
    # 2 : 1 in ONE axis only: the general form, not a two-tap area mean
    y = planes(9, 64, 66)
    got = U.resize_u8(y, 32, 32)
    ix0, ix1, wx0, wx1 = U.axis_taps(66, 32)
    assert not (wx1 == 0.5).all()                                # 66 -> 32 is not 2 : 1
    b0, b1 = U.fixed_weights(*U.axis_taps(64, 32)[2:])
    assert (b0 == 1024).all() and (b1 == 1024).all()
    t = y.astype(np.int32)
    a0, a1 = U.fixed_weights(wx0, wx1)
    d = (t[:, :, ix0] * a0 + t[:, :, ix1] * a1) >> 4
    want = (((1024 * d[:, 0::2]) >> 16) + ((1024 * d[:, 1::2]) >> 16) + 2) >> 2
    assert np.array_equal(got, want.astype(np.uint8))
    assert U.is_area(64, 64, 32, 32) and not U.is_area(64, 66, 32, 32) and not U.is_area(66, 64, 32, 32)


# --------------------------------------------------------------------------- the float flavour
@pytest.mark.parametrize("src,size", RESIZES)
def test_float_flavour_within_the_sibling_bound(src, size):
    x = planes(11, *src).astype(np.float32)
    got = U.resize_f32(x, *size)
    ref = U.resize_f32(x, *size, dtype=np.float64)
    M = U.tap_magnitude(x, *size)
    k = 2.25 if U.is_area(*src, *size) else 4.0
    assert (np.abs(got.astype(np.float64) - ref) <= k * 2.0 ** -24 * M).all()


def test_normalise_after_differs_from_normalise_before():
    img = U.noise(13, 1, 45, 70)
    c = U.CENTERNET
    after = U.letterbox(img, (36, 56), (64, 64), (0, 0), 1, c["mean"], c["std"], c["to_rgb"], c["pad"])
    before = U.normalise_before(img, (36, 56), (64, 64), (0, 0), c["mean"], c["std"], c["to_rgb"])
    inside = (slice(None), slice(None), slice(0, 36), slice(0, 56))
    differ = int((after[inside].view(np.uint32) != before[inside].view(np.uint32)).sum())
    print(f"normalise after / before the resize: {differ} of {after[inside].size} fp32 values differ")
    assert differ > 0
    assert np.abs(after[inside] - before[inside]).max() < 1e-5          # the same picture, another rounding order
    # and the padding is the normalised pad value, not zero
    pad = ((np.float32(0) - np.asarray(c["mean"], np.float32)) * (1.0 / np.asarray(c["std"])).astype(np.float32))
    assert np.array_equal(after[0, :, 63, 63], pad.astype(np.float32))


def test_restatement_pastes_and_pads_in_source_channel_order():
    img = U.noise(17, 2, 5, 6)
    out = U.letterbox(img, (5, 6), (8, 9), (2, 1), 0, (0, 0, 0), (1, 1, 1), True, (10.0, 20.0, 30.0))
    assert out.shape == (2, 3, 8, 9)
    assert np.array_equal(out[:, :, 2:7, 1:7], img.transpose(0, 3, 1, 2)[:, ::-1].astype(np.float32))
    assert (out[:, 0, 0, 0] == 30.0).all() and (out[:, 2, 7, 8] == 10.0).all()    # the swap reaches the pad value too


# --------------------------------------------------------------------------- the C entry
def test_status_codes_without_a_gpu():
    from bevformer_tensorrt_amd.utils import lib as L
    f = L.load_library().bevops_image_letterbox
    D3 = ctypes.c_double * 3
    mean, std, pad = D3(1, 2, 3), D3(1, 1, 1), D3(114, 114, 114)
    img = np.zeros((1, 8, 8, 3), np.uint8)
    out = np.zeros((1, 3, 32, 32), np.float32)
    p, o = img.ctypes.data, out.ctypes.data

    def call(arith=0, images=p, out_dtype=L.F32, output=o, N=1, H0=8, W0=8, Hs=4, Ws=4, Hp=32, Wp=32, oy=0, ox=0, pd=pad,
             m=mean, s=std):
        return f(arith, images, out_dtype, output, N, H0, W0, Hs, Ws, Hp, Wp, oy, ox, pd, m, s, 0, 0, None)

    assert call(images=None) == L.BAD_PARAM and call(output=None) == L.BAD_PARAM
    assert call(m=None) == L.BAD_PARAM and call(s=None) == L.BAD_PARAM and call(pd=None) == L.BAD_PARAM
    assert call(N=0) == L.BAD_PARAM and call(H0=0) == L.BAD_PARAM and call(Ws=0) == L.BAD_PARAM and call(Hp=0) == L.BAD_PARAM
    assert call(Hp=3) == L.BAD_PARAM and call(Wp=3) == L.BAD_PARAM                     # the paste leaves the canvas
    assert call(oy=-1) == L.BAD_PARAM and call(ox=-1) == L.BAD_PARAM
    assert call(oy=29) == L.BAD_PARAM and call(ox=29) == L.BAD_PARAM                   # 29 + 4 > 32
    assert call(s=D3(1, 0, 1)) == L.BAD_PARAM and call(s=D3(1, -1, 1)) == L.BAD_PARAM
    assert call(output=o + 2) == L.BAD_PARAM and call(output=o + 1, out_dtype=L.F16) == L.BAD_PARAM
    assert call(arith=2) == L.NOT_SUPPORTED and call(arith=-1) == L.NOT_SUPPORTED
    assert call(out_dtype=L.I8) == L.NOT_SUPPORTED and call(out_dtype=L.U8) == L.NOT_SUPPORTED
    # outside the domain: one tile's window above 64 KiB (a 64-fold reduction of a wide image)
    assert call(H0=4096, W0=4096, Hs=64, Ws=64, Hp=64, Wp=64) == L.NOT_SUPPORTED
    assert call(arith=1, H0=4096, W0=4096, Hs=64, Ws=64, Hp=64, Wp=64) == L.NOT_SUPPORTED
    assert call(N=70000) == L.NOT_SUPPORTED
    assert call(Hp=(1 << 20) + 8) == L.NOT_SUPPORTED
    assert (out == 0).all()


def test_exports_and_argument_checks():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd import functions as F
    from bevformer_tensorrt_amd.utils import lib as L
    for name in ("DETECT2D_IMAGE_PIPELINES", "keep_ratio_size", "yolox_test_geometry", "centernet_test_geometry",
                 "image_letterbox"):
        assert name in F.__all__ and hasattr(bev, name)
    assert "bevops_image_letterbox" in L.SIGNATURES
    handle = L.load_library()
    assert handle.bevops_query(b"bevops_image_letterbox") == ctypes.cast(handle.bevops_image_letterbox, ctypes.c_void_p).value
    with pytest.raises(AssertionError):
        bev.image_letterbox(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), bev.yolox_test_geometry(4, 4), "yolox")   # not on the GPU
