"""The BEVFormer tiny / small camera front end without a GPU: `scale_lidar2img` / `scaled_size` against what the
reference's own RandomScaleImageMultiViewImage computed (tests/golden/image_scale.npz); the numpy restatement of the
resize (tests/util_image_scale.py) against its own float64 evaluation within a derived bound and against
torch.nn.functional.interpolate in double (an independent statement of the sampling geometry); the visibility of a
contracted evaluation; scale = 1; the status codes of the C entry; the exports."""
import ctypes

import numpy as np
import pytest
import torch

import util_image_scale as U
from conftest import golden

EPS = 2.0 ** -24          # unit roundoff of float32


@pytest.fixture(scope="module")
def gold():
    return golden("image_scale")


def test_scale_lidar2img_and_scaled_size_match_the_reference(gold):
    import bevformer_tensorrt_amd as bev
    l2i = gold["lidar2img"]
    for s in gold["scales"]:
        tag = f"s{int(s * 10):02d}"
        want64, want32 = gold[f"{tag}_prod64"], gold[f"{tag}_prod32"]
        assert np.array_equal(want64.astype(np.float32).view(np.uint32), want32.view(np.uint32))
        for src in (torch.from_numpy(l2i), torch.from_numpy(l2i)[None], l2i):
            got = bev.scale_lidar2img(src, float(s))
            assert got.dtype == torch.float32 and tuple(got.shape) == tuple(np.shape(src))
            assert np.array_equal(got.numpy().reshape(6, 4, 4).view(np.uint32), want32.view(np.uint32))
        assert np.array_equal(U.scale_lidar2img(l2i, float(s)).view(np.uint32), want32.view(np.uint32))
        for (h, w), (xs, ys) in zip(gold["sizes"], gold[f"{tag}_requested"]):
            assert bev.scaled_size(int(h), int(w), float(s)) == (int(ys), int(xs)) == U.scaled_size(int(h), int(w), float(s))
    assert bev.scaled_size(900, 1600, 0.8) == (720, 1280) and bev.scaled_size(900, 1600, 0.5) == (450, 800)
    assert bev.scaled_size(900, 1600, None) == (900, 1600)
    # the float64 rule is observable at 0.8: a float32-by-float32 product gives other matrices
    naive = (l2i.astype(np.float32)[:, :2] * np.float32(0.8)).astype(np.float32)
    assert (naive != gold["s08_prod32"][:, :2]).any()
    assert torch.equal(bev.scale_lidar2img(torch.from_numpy(l2i), None), torch.from_numpy(l2i).float())


def test_pipelines_are_the_three_configs():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.bevformer import CONFIGS
    P = bev.BEVFORMER_IMAGE_PIPELINES
    assert P["tiny"] == dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True, scale=0.5,
                             size_divisor=32)
    assert P["small"] == dict(mean=[103.530, 116.280, 123.675], std=[1.0, 1.0, 1.0], to_rgb=False, scale=0.8,
                              size_divisor=32)
    assert P["base"] == dict(mean=[103.530, 116.280, 123.675], std=[1.0, 1.0, 1.0], to_rgb=False, scale=None,
                             size_divisor=32)
    for name, p in P.items():      # 900 x 1600 through each pipeline is the model's input size
        assert bev.padded_size(*bev.scaled_size(900, 1600, p["scale"]), p["size_divisor"]) == tuple(CONFIGS[name]["image"])


def _cases():
    for name, (src, dst) in U.CASES.items():
        yield name, src, dst
    yield "nuscenes08", (900, 1600), (720, 1280)
    yield "nuscenes05", (900, 1600), (450, 800)


@pytest.mark.parametrize("name,src,dst", list(_cases()), ids=[c[0] for c in _cases()])
def test_restatement_within_bound_of_float64(name, src, dst):
    """|float32 restatement - float64 evaluation with the same taps and float32 weights| <= 4 u M, u = 2^-24, M the
    largest magnitude among the four normalised taps.  A pass fl(fl(a w0) + fl(b w1)) has three roundings: the two
    products err by at most u (|a| w0 + |b| w1) <= u M (the weights sum to one), the sum by at most u M: 2 u M.  The
    vertical pass carries the horizontal one's 2 u M through weights that sum to one and adds its own 2 u M.
    Area form: the three sums are at most 2 M, 3 M and 4 M in magnitude, so they err by at most u (2 + 3 + 4) M, and
    the exact * 0.25 leaves 2.25 u M.  The largest ratio seen is printed."""
    n = 1 if src[0] >= 900 else 2
    worst = 0.0
    for dtype in (np.uint8, np.float32):
        for norm in (U.BASE_NORM, U.TINY_NORM):
            x = U.normalized(U.noise(7, n, *src, dtype=dtype), **norm)
            got = U.resize(x, *dst)
            assert got.dtype == np.float32 and got.shape == x.shape[:2] + dst
            want = U.resize(x, *dst, dtype=np.float64)
            M = U.tap_magnitude(x, *dst).astype(np.float64)
            k = 2.25 if U.is_area(*src, *dst) else 4.0
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= k * EPS * M).all(), (name, float((err / np.maximum(M, 1e-30)).max() / EPS))
            worst = max(worst, float((err / np.maximum(M, 1e-30)).max() / EPS))
            if src[0] >= 900 and dtype == np.float32:
                break
    print(f"{name}: largest |error| / (2^-24 M) = {worst:.3f}")


def _interpolate64(x, dst):
    return torch.nn.functional.interpolate(torch.from_numpy(x).double(), size=dst, mode="bilinear",
                                           align_corners=False).numpy()


def _ulp32(v):
    return float(np.spacing(np.float32(v)))


@pytest.mark.parametrize("src,dst,exact", [((45, 70), (36, 56), True), ((90, 160), (72, 128), True),
                                           ((90, 160), (45, 80), True), ((45, 70), (22, 35), False),
                                           ((37, 53), (29, 42), False), ((33, 65), (9, 19), False),
                                           ((20, 24), (30, 36), False), ((46, 71), (23, 35), False)])
def test_sampling_geometry_against_torch_interpolate(src, dst, exact):
    """The float64 evaluation with the restatement's taps and float32 weights against torch's bilinear interpolation in
    double.  torch's source position is (d + 0.5) * (in / out) - 0.5 in double; the restatement's scale
    1 / (out / in) is the same double for these sizes and its position is rounded to float32 ONCE: where that rounding
    is exact the two agree exactly, elsewhere a weight moves by at most half an ulp32 of the position (< in) per axis,
    times |a - b| <= 2 M: (ulp32(W0) + ulp32(H0)) M.  (The area form is not bilinear sampling: general path here.)"""
    x = U.normalized(U.noise(11, 2, *src), **U.TINY_NORM)
    ix0, ix1, wx0, wx1 = U.axis_taps(src[1], dst[1])
    iy0, iy1, wy0, wy1 = U.axis_taps(src[0], dst[0])
    x64 = x.astype(np.float64)
    h = x64[..., :, ix0] * wx0.astype(np.float64) + x64[..., :, ix1] * wx1.astype(np.float64)
    ours = h[..., iy0, :] * wy0.astype(np.float64)[:, None] + h[..., iy1, :] * wy1.astype(np.float64)[:, None]
    want = _interpolate64(x, dst)
    M = np.abs(x).max()
    diff = float(np.abs(ours - want).max())
    print(f"{src} -> {dst}: max |difference| = {diff / M:.3e} M")
    if exact:
        assert diff == 0.0           # positions and weights are exact in float32: the same double arithmetic
    else:
        assert diff <= (_ulp32(src[1]) + _ulp32(src[0])) * M


def test_a_contracted_evaluation_is_visible():
    x = U.normalized(U.noise(7, 2, 45, 70), **U.BASE_NORM)
    plain, fused = U.resize(x, 36, 56), U.resize(x, 36, 56, contract=True)
    differ = int((plain != fused).sum())
    print(f"contracted evaluation differs in {differ} of {plain.size} values")
    assert differ > 0
    assert np.abs(plain.astype(np.float64) - fused).max() <= 4 * EPS * np.abs(x).max()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("norm", ["base", "tiny"])
def test_scale_one_is_normalize_pad(dtype, norm):
    from oracle.image_ref import image_normalize_pad
    img = U.noise(3, 2, 45, 70, dtype=dtype)
    want = image_normalize_pad(img, **U.NORMS[norm])
    got = U.normalize_resize_pad(img, (45, 70), **U.NORMS[norm])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_tap_rules():
    i0, i1, w0, w1 = U.axis_taps(1600, 1280)                  # 0.8: scale 1.25 exactly, f in {0.125, 0.375, ...}
    assert i0[0] == 0 and w1[0] == np.float32(0.125) and i0[-1] == 1598 and i1[-1] == 1599
    i0, i1, w0, w1 = U.axis_taps(24, 36)                      # up-scale: both clamps
    assert i0[0] == 0 and w1[0] == 0 and w0[0] == 1           # position -1/6 -> clamped
    assert i0[-1] == 23 and i1[-1] == 23 and w1[-1] == 0
    i0, i1, w0, w1 = U.axis_taps(7, 3)
    assert (i1 <= 6).all() and (w0 + w1 == 1).all()
    assert U.axis_taps(1, 1)[0].tolist() == [0]


def test_status_codes_without_a_gpu():
    from bevformer_tensorrt_amd.utils import lib as L
    handle = L.load_library()
    f = handle.bevops_image_normalize_resize_pad
    D3 = ctypes.c_double * 3
    mean, std = D3(1, 2, 3), D3(1, 1, 1)
    img = np.zeros((1, 8, 8, 3), np.uint8)
    out = np.zeros((1, 3, 32, 32), np.float32)
    p, o = img.ctypes.data, out.ctypes.data

    def call(in_dtype=L.U8, images=p, out_dtype=L.F32, output=o, N=1, H0=8, W0=8, Hs=4, Ws=4, Hp=32, Wp=32, m=mean,
             s=std):
        return f(in_dtype, images, out_dtype, output, N, H0, W0, Hs, Ws, Hp, Wp, m, s, 0, 0, None)

    assert call(images=None) == L.BAD_PARAM and call(output=None) == L.BAD_PARAM
    assert call(m=None) == L.BAD_PARAM and call(s=None) == L.BAD_PARAM
    assert call(N=0) == L.BAD_PARAM and call(H0=0) == L.BAD_PARAM and call(Ws=0) == L.BAD_PARAM
    assert call(Hp=3) == L.BAD_PARAM and call(Wp=3) == L.BAD_PARAM
    assert call(s=D3(1, 0, 1)) == L.BAD_PARAM and call(s=D3(1, -1, 1)) == L.BAD_PARAM
    assert call(in_dtype=L.F16) == L.NOT_SUPPORTED and call(in_dtype=L.I8) == L.NOT_SUPPORTED
    assert call(out_dtype=L.I8) == L.NOT_SUPPORTED and call(out_dtype=L.U8) == L.NOT_SUPPORTED
    # outside the domain: one tile's window above 64 KiB (a 64-fold reduction of a wide image)
    assert call(H0=4096, W0=4096, Hs=64, Ws=64, Hp=64, Wp=64) == L.NOT_SUPPORTED
    assert call(N=70000) == L.NOT_SUPPORTED


def test_exports_and_argument_checks():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd import functions as F
    from bevformer_tensorrt_amd.quantization import Int8PluginOps
    from bevformer_tensorrt_amd.utils import lib as L
    for name in ("BEVFORMER_IMAGE_PIPELINES", "scaled_size", "scale_lidar2img", "image_normalize_resize_pad"):
        assert name in F.__all__ and hasattr(bev, name)
    assert "bevops_image_normalize_resize_pad" in L.SIGNATURES
    assert "image_normalize_resize_pad" in Int8PluginOps._PASS
    with pytest.raises(AssertionError):
        bev.image_normalize_resize_pad(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), scale=0.5)     # not on the GPU
