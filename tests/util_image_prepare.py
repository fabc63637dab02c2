"""numpy restatement of what BEVDet's camera front end computes (test infrastructure only; independent of the C plan
builder): Pillow's `Image.resize` with the default antialiased bicubic filter on an 8-bit RGB image
(Pillow src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc,
ImagingResampleVertical_8bpc), then `crop` and the left-right flip of PrepareImageInputs.img_transform_core
(third_party/bev_mmdet3d/datasets/pipelines/loading.py:747-754).

Per axis: scale = in / out, filterscale = max(scale, 1), support = 2 filterscale, ksize = ceil(support) * 2 + 1; for
output index xx: center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support
+ 0.5), in) - xmin; tap x weighs bicubic((x + xmin - center + 0.5) * (1 / filterscale)), a = -0.5; the weights are
summed in tap order in double, each divided by the sum and rounded as int(+-0.5 + w * 2^22) (truncation, the sign of
w).  A pass is clip(0, 255, (2^21 + sum pixel * k) >> 22); the horizontal pass runs first and its uint8 result feeds
the vertical pass."""
import numpy as np

PRECISION_BITS = 22
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)      # mmlabNormalize, loading.py:694-695

# (source (H, W), data_config, flip, scale) -> expected (resize, resize_dims, crop): the fixture cases of
# tests/golden/image_prepare.npz, by name
CASES = {
    "default": ((90, 160), dict(input_size=(24, 70), crop_h=(0.0, 0.0), resize_test=0.0), None, None,
                (0.4375, (70, 39), (0, 15, 70, 39))),
    "resize_test_flip": ((90, 160), dict(input_size=(24, 70), crop_h=(0.0, 0.0), resize_test=0.03), True, None,
                         (None, None, (2, 18, 72, 42))),
    "crop_h_scale": ((90, 160), dict(input_size=(24, 70), crop_h=(0.1, 0.1), resize_test=0.0), None, 0.04,
                     (None, None, (3, 13, 73, 37))),
    "upscale": ((40, 64), dict(input_size=(48, 96), crop_h=(0.0, 0.0), resize_test=0.0), None, None,
                (1.5, (96, 60), None)),
    "odd_flip": ((37, 53), dict(input_size=(16, 23), crop_h=(0.0, 0.0), resize_test=0.0), True, None,
                 (None, (23, 16), (0, 0, 23, 16))),
}
DATA_CONFIG_R50 = dict(input_size=(256, 704), src_size=(900, 1600), crop_h=(0.0, 0.0), resize_test=0.0)


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """-> (kk [out, ksize] int64, zero behind a row's taps; bounds [out, 2] = (xmin, taps); ksize)."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), np.int64)
    bounds = np.zeros((out_size, 2), np.int64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            v = v * (1 << PRECISION_BITS)
            kk[xx, x] = int(-0.5 + v) if v < 0 else int(0.5 + v)
        bounds[xx] = xmin, xmax
    return kk, bounds, ksize


def pass1d(img, out_size, keep=None):
    """One pass along axis 1 of img [A, in, C] uint8 -> [A, out, C] uint8; keep = (lo, hi) computes only those output
    indices (-> [A, hi - lo, C])."""
    kk, b, _ = coeffs(img.shape[1], out_size)
    lo, hi = (0, out_size) if keep is None else keep
    out = np.empty((img.shape[0], hi - lo, img.shape[2]), np.uint8)
    wide = img.astype(np.int64)
    for xx in range(lo, hi):
        x0, n = b[xx]
        acc = (wide[:, x0:x0 + n] * kk[xx, :n][None, :, None]).sum(1) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < (1 << 31)
        out[:, xx - lo] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img, W, H, crop=None):
    """Image.resize((W, H)) of img [H0, W0, 3] uint8: horizontal pass, then vertical pass on its uint8 result.
    crop = (x0, y0, x1, y1): only that part of the result."""
    x0, y0, x1, y1 = (0, 0, W, H) if crop is None else crop
    assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H
    t = pass1d(img, W, (x0, x1))
    return np.ascontiguousarray(pass1d(t.transpose(1, 0, 2), H, (y0, y1)).transpose(1, 0, 2))


def resize_vertical_first(img, W, H):
    """The other pass order (NOT what PIL computes): the generator asserts that it differs."""
    t = pass1d(img.transpose(1, 0, 2), H).transpose(1, 0, 2)
    return np.ascontiguousarray(pass1d(np.ascontiguousarray(t), W))


def prepare(img, resize_dims, crop, flip):
    """img_transform_core at rotate = 0: the uint8 canvas [fH, fW, 3]."""
    c = resize(img, resize_dims[0], resize_dims[1], crop)
    return np.ascontiguousarray(c[:, ::-1]) if flip else c


def ref_augmentation(H, W, data_config, flip=None, scale=None):
    """sample_augmentation, is_train=False (loading.py:779-792), restated for inputs the fixture does not hold."""
    fH, fW = data_config["input_size"]
    resize_ = float(fW) / float(W) + (scale if scale is not None else data_config.get("resize_test", 0.0))
    dims = (int(W * resize_), int(H * resize_))
    crop_h = int((1 - np.mean(data_config["crop_h"])) * dims[1]) - fH
    crop_w = int(max(0, dims[0] - fW) / 2)
    return resize_, dims, (crop_w, crop_h, crop_w + fW, crop_h + fH), bool(flip), 0


def noise(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def checkerboard(n, h, w, block=5):
    """0 / 255 blocks, the three channels differing (inverted; shifted by 3 columns), camera i shifted by 2 i rows."""
    yy, xx = np.mgrid[:h, :w]
    out = []
    for i in range(n):
        a = ((((yy + 2 * i) // block + xx // block) % 2) * 255).astype(np.uint8)
        out.append(np.stack([a, 255 - a, np.roll(a, 3, 1)], -1))
    return np.stack(out)


def normalized(canvas):
    """mmlabNormalize of uint8 canvases [N, fH, fW, 3] -> float32 [N, 3, fH, fW] (oracle/image_ref.py, size_divisor 1)."""
    from oracle.image_ref import image_normalize_pad
    return image_normalize_pad(canvas, mean=MEAN, std=STD, to_rgb=True, size_divisor=1)
