"""numpy restatement of bevops_image_letterbox (test infrastructure only): the test pipelines of the two 2-D detectors --
YOLOX: Resize(keep_ratio) on uint8 -> Pad(pad_to_square, 114); CenterNet: Resize(keep_ratio) on float32 ->
RandomCenterCropPad(test_mode) -> Pad -> Normalize -- as resize, paste at an offset into a constant canvas, normalise
(design/letterbox.md).  The resize is the published operation order of cv::resize(INTER_LINEAR), written from its
specification: the 8-bit fixed-point form (11-bit coefficients, the vertical pass on D >> 4, the 2 : 1 area switch) and the
float32 form of tests/util_image_scale.py.  PARITY UNPINNED against cv2 / mmcv / mmdet themselves: none is installed.  The
HIP kernel is held bit-exact against THIS."""
import numpy as np

from util_image_scale import axis_taps, is_area, noise, resize as resize_f32, tap_magnitude   # noqa: F401

YOLOX = dict(arith=0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), to_rgb=False, pad=(114.0, 114.0, 114.0))
CENTERNET = dict(arith=1, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), to_rgb=True, pad=(0.0, 0.0, 0.0))
PIPELINES = {"yolox": YOLOX, "centernet": CENTERNET}

COEF_BITS = 11
COEF_SCALE = np.float32(1 << COEF_BITS)

# Distance of the fixed-point form from the float64 bilinear interpolation with the same taps, in grey levels
# (design/letterbox.md, "The bound"): per pass the two rounded coefficients are off by at most 2^-12 each, on values of at
# most 255 (the second pass: 255 (1 + 2^-11), the coefficients of the first may sum to 2049 / 2048); D >> 4 drops less
# than 2^-7; each >> 16 drops less than a quarter level; (. + 2) >> 2 rounds by at most half a level.
FIXED_BOUND = 2 * 255 * 2.0 ** -11 * (1 + 2.0 ** -11) + 2.0 ** -7 + 2 * 0.25 + 0.5      # 1.2570


def fixed_weights(w0, w1):
    """float32 (1 - f, f) -> int32 (a0, a1) = rint of the float32 products with 2048, half to even."""
    a0 = np.rint((w0.astype(np.float32) * COEF_SCALE).astype(np.float32)).astype(np.int32)
    a1 = np.rint((w1.astype(np.float32) * COEF_SCALE).astype(np.float32)).astype(np.int32)
    return a0, a1


def resize_u8(x, Hs, Ws, clip=True):
    """x [..., H0, W0] uint8 -> [..., Hs, Ws]: cv::resize's 8-bit INTER_LINEAR.  clip=False returns the int32 result before
    the uint8 cast (the tests assert that it lies in 0 .. 255)."""
    H0, W0 = x.shape[-2:]
    s = x.astype(np.int32)
    if is_area(H0, W0, Hs, Ws):
        r = (s[..., 0::2, 0::2] + s[..., 0::2, 1::2] + s[..., 1::2, 0::2] + s[..., 1::2, 1::2] + 2) >> 2
    else:
        ix0, ix1, wx0, wx1 = axis_taps(W0, Ws)
        iy0, iy1, wy0, wy1 = axis_taps(H0, Hs)
        a0, a1 = fixed_weights(wx0, wx1)
        b0, b1 = fixed_weights(wy0, wy1)
        d = (s[..., :, ix0] * a0 + s[..., :, ix1] * a1) >> 4                   # horizontal pass, then the >> 4
        r = (((b0[:, None] * d[..., iy0, :]) >> 16) + ((b1[:, None] * d[..., iy1, :]) >> 16) + 2) >> 2
    return r.astype(np.uint8) if clip else r


def bilinear_f64(x, Hs, Ws):
    """The same float32 taps and weights evaluated in float64 (no area switch): the reference of the error bounds."""
    H0, W0 = x.shape[-2:]
    ix0, ix1, wx0, wx1 = axis_taps(W0, Ws)
    iy0, iy1, wy0, wy1 = axis_taps(H0, Hs)
    x = x.astype(np.float64)
    wx1, wy1 = wx1.astype(np.float64), wy1.astype(np.float64)
    h = x[..., :, ix0] * (1.0 - wx1) + x[..., :, ix1] * wx1
    return h[..., iy0, :] * (1.0 - wy1[:, None]) + h[..., iy1, :] * wy1[:, None]


def normalise(x, mean, std):
    """x float32 [N, 3, H, W] in OUTPUT channel order: fl(x - float32(mean)), fl(. * float32(1 / float64(std)))."""
    m = np.asarray(mean, np.float64).astype(np.float32).reshape(1, 3, 1, 1)
    inv = (1.0 / np.asarray(std, np.float64)).astype(np.float32).reshape(1, 3, 1, 1)
    return ((x - m).astype(np.float32) * inv).astype(np.float32)


def resized(images, size, arith, to_rgb):
    """[N, H0, W0, 3] uint8 -> float32 [N, 3, Hs, Ws] in OUTPUT channel order, not yet normalised."""
    x = np.ascontiguousarray(images.transpose(0, 3, 1, 2))
    if to_rgb:
        x = x[:, ::-1]
    if arith == 0:
        return resize_u8(x, *size).astype(np.float32)
    return resize_f32(x.astype(np.float32), *size)


def letterbox(images, size, canvas, offset, arith, mean, std, to_rgb, pad):
    """images [N, H0, W0, 3] uint8 (BGR) -> float32 [N, 3, Hp, Wp]: the restatement.  `pad` is in the SOURCE channel
    order, like the canvas the pipelines fill before their channel swap."""
    (Hs, Ws), (Hp, Wp), (oy, ox) = size, canvas, offset
    p = np.asarray(pad, np.float64).astype(np.float32)
    if to_rgb:
        p = p[::-1]
    out = np.empty((images.shape[0], 3, Hp, Wp), np.float32)
    out[:] = p.reshape(1, 3, 1, 1)
    out[:, :, oy:oy + Hs, ox:ox + Ws] = resized(images, size, arith, to_rgb)
    return normalise(out, mean, std)


def normalise_before(images, size, canvas, offset, mean, std, to_rgb):
    """The OTHER order (bevops_image_normalize_resize_pad's): every tap normalised, then the float32 resize, zero padding."""
    (Hs, Ws), (Hp, Wp), (oy, ox) = size, canvas, offset
    x = np.ascontiguousarray(images.transpose(0, 3, 1, 2))
    if to_rgb:
        x = x[:, ::-1]
    r = resize_f32(normalise(x.astype(np.float32), mean, std), Hs, Ws)
    out = np.zeros((images.shape[0], 3, Hp, Wp), np.float32)
    out[:, :, oy:oy + Hs, ox:ox + Ws] = r
    return out


def keep_ratio_size(H0, W0, img_scale=(640, 640)):
    s = min(max(img_scale) / max(H0, W0), min(img_scale) / min(H0, W0))
    return int(H0 * s + 0.5), int(W0 * s + 0.5)
