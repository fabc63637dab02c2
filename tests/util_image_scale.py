"""numpy restatement of bevops_image_normalize_resize_pad (test infrastructure only): NormalizeMultiviewImage ->
RandomScaleImageMultiViewImage -> PadMultiViewImage of the BEVFormer tiny / small test pipelines, with the resize in the
published operation order of cv::resize(INTER_LINEAR) on a float32 image, written from its specification
(design/image_scale.md).  PARITY UNPINNED against cv2 / mmcv themselves: neither is installed, and the last bit of cv2's
float32 result depends on whether its build contracts a * w0 + b * w1 into a fused multiply-add.  Here every step is a
float32 operation of its own; the HIP kernel is held bit-exact against THIS."""
import numpy as np

from oracle.image_ref import image_normalize_pad as _normalize_pad

BASE_NORM = dict(mean=(103.530, 116.280, 123.675), std=(1.0, 1.0, 1.0), to_rgb=False)
TINY_NORM = dict(mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), to_rgb=True)
NORMS = {"base": BASE_NORM, "tiny": TINY_NORM}

# (H0, W0) -> (Hs, Ws); the cases of the issue: 0.8 and 0.5 on an even size, the area form, 2 : 1 in one axis only,
# an odd size, a strong reduction, an up-scale (both clamps), two degenerate sizes
CASES = {
    "s08": ((45, 70), (36, 56)),
    "s05": ((45, 70), (22, 35)),
    "area": ((46, 70), (23, 35)),
    "half_one_axis": ((46, 71), (23, 35)),
    "odd08": ((37, 53), (29, 42)),
    "s03": ((33, 65), (9, 19)),
    "up": ((20, 24), (30, 36)),
    "small": ((3, 5), (2, 4)),
    "one_row": ((1, 7), (1, 3)),
}


def scaled_size(H0, W0, scale):
    return int(H0 * scale), int(W0 * scale)


def padded(h, w, divisor=32):
    return -(-h // divisor) * divisor, -(-w // divisor) * divisor


def noise(seed, n, H, W, dtype=np.uint8):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    if dtype == np.uint8:
        return img
    return (img.astype(np.float32) + rng.random(img.shape, dtype=np.float32) * np.float32(0.5)).astype(np.float32)


def axis_taps(n_in, n_out):
    """-> (i0, i1 int64 [n_out], w0, w1 float32 [n_out]) of one axis."""
    scale = 1.0 / (float(n_out) / float(n_in))
    d = np.arange(n_out, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)           # double arithmetic, ONE rounding
    i = np.floor(f).astype(np.int64)
    f = (f - i.astype(np.float32)).astype(np.float32)          # exact
    lo, hi = i < 0, i >= n_in - 1
    i[lo], f[lo] = 0, 0
    i[hi], f[hi] = n_in - 1, 0
    return i, np.minimum(i + 1, n_in - 1), (np.float32(1) - f).astype(np.float32), f


def is_area(H0, W0, Hs, Ws):
    return H0 == 2 * Hs and W0 == 2 * Ws


def normalized(images, mean, std, to_rgb):
    """[N, H0, W0, 3] -> float32 [N, 3, H0, W0]: every source pixel as bevops_image_normalize_pad normalises it."""
    return _normalize_pad(images, mean=mean, std=std, to_rgb=to_rgb, size_divisor=1)


def resize(x, Hs, Ws, contract=False, dtype=np.float32):
    """x [..., H0, W0] float32 (normalised planes) -> [..., Hs, Ws]: horizontal pass first, fl(fl(a w0) + fl(b w1)) per
    pass; 2 : 1 in both axes: fl(fl(fl(fl(a + b) + c) + d) * 0.25).  dtype=np.float64 evaluates the same float32 weights
    and taps in double (the reference of the error bound); contract=True rounds a * w0 + b * w1 ONCE per pass, as a
    build that fuses the multiply-adds would -- evaluated in float64, exact up to double rounding of a 48-bit sum."""
    H0, W0 = x.shape[-2:]
    x = x.astype(dtype)
    if is_area(H0, W0, Hs, Ws) and not contract:
        a, b, c, d = x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]
        return ((((a + b).astype(dtype) + c).astype(dtype) + d).astype(dtype) * dtype(0.25)).astype(dtype)
    ix0, ix1, wx0, wx1 = axis_taps(W0, Ws)
    iy0, iy1, wy0, wy1 = axis_taps(H0, Hs)

    def one(a, b, w0, w1):
        if contract:
            return (a.astype(np.float64) * w0.astype(np.float64) + b.astype(np.float64) * w1.astype(np.float64)).astype(np.float32)
        return ((a * w0.astype(dtype)).astype(dtype) + (b * w1.astype(dtype)).astype(dtype)).astype(dtype)

    h = one(x[..., :, ix0], x[..., :, ix1], wx0, wx1)
    return one(h[..., iy0, :], h[..., iy1, :], wy0[:, None], wy1[:, None])


def tap_magnitude(x, Hs, Ws):
    """Largest |value| among the four source taps of every output pixel: the M of the error bounds."""
    H0, W0 = x.shape[-2:]
    a = np.abs(x)
    if is_area(H0, W0, Hs, Ws):
        return np.maximum(np.maximum(a[..., 0::2, 0::2], a[..., 0::2, 1::2]), np.maximum(a[..., 1::2, 0::2], a[..., 1::2, 1::2]))
    ix0, ix1, _, _ = axis_taps(W0, Ws)
    iy0, iy1, _, _ = axis_taps(H0, Hs)
    h = np.maximum(a[..., :, ix0], a[..., :, ix1])
    return np.maximum(h[..., iy0, :], h[..., iy1, :])


def normalize_resize_pad(images, size, mean, std, to_rgb, size_divisor=32):
    """images [N, H0, W0, 3] uint8 / float32 (BGR) -> float32 [N, 3, Hp, Wp]: the restatement."""
    Hs, Ws = size
    r = resize(normalized(images, mean, std, to_rgb), Hs, Ws)
    Hp, Wp = padded(Hs, Ws, size_divisor)
    out = np.zeros(r.shape[:2] + (Hp, Wp), np.float32)
    out[..., :Hs, :Ws] = r
    return out


def scale_lidar2img(l2i, scale):
    """float64 diag(s, s, 1, 1) @ l2i, one rounding to float32 (transform_3d.py:426-433, evaluate_trt.py:131-132)."""
    sf = np.eye(4)
    sf[0, 0] *= scale
    sf[1, 1] *= scale
    return np.stack([(sf @ m) for m in np.asarray(l2i, np.float64).reshape(-1, 4, 4)]).astype(np.float32).reshape(np.shape(l2i))


def realistic_lidar2img(seed=0):
    """Six nuScenes-like lidar2img matrices (float64): intrinsics of about 1 260 px focal length at 1600 x 900, cameras
    on a ring, small random offsets, so that rows 0 and 1 hold values of 10 .. 2 000 with full mantissas."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(6):
        yaw = np.deg2rad(60.0 * k) + rng.normal(0, 0.02)
        fwd = np.array([np.cos(yaw), np.sin(yaw), rng.normal(0, 0.01)])
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])                       # lidar -> camera rotation
        t = -R @ (np.array([1.5 * np.cos(yaw), 1.5 * np.sin(yaw), 1.6]) + rng.normal(0, 0.05, 3))
        K = np.eye(4)
        K[0, 0], K[1, 1] = 1260.0 + rng.normal(0, 8), 1260.0 + rng.normal(0, 8)
        K[0, 2], K[1, 2] = 800.0 + rng.normal(0, 20), 450.0 + rng.normal(0, 20)
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = R, t
        out.append(K @ E)
    return np.stack(out)
