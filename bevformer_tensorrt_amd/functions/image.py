"""image_normalize_pad -- the camera-image front end of the frame loop: the
reference's NormalizeMultiviewImage + PadMultiViewImage(size_divisor=32) + DefaultFormatBundle3D
(configs/bevformer/bevformer_base.py:11,228-231) as one HIP pass over the raw images."""
import ctypes

import numpy as np
import torch

from ..utils import lib as _lib

IMG_NORM_CFG = dict(mean=[103.530, 116.280, 123.675], std=[1.0, 1.0, 1.0], to_rgb=False)   # bevformer_base.py:11


def padded_size(h, w, divisor=32):
    """mmcv.impad_to_multiple: bottom / right padding to the next multiple of `divisor`."""
    return -(-h // divisor) * divisor, -(-w // divisor) * divisor


def _dense_out(out, shape, dtype, device, channels_last, any_gpu=False):
    """`out` if given, after the check that it is a dense `shape` tensor in the asked memory format on `device` (any_gpu:
    on any GPU); else a new one of `dtype`."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device,
                           memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    if tuple(out.shape) != shape or not (out.is_cuda if any_gpu else out.device == device) or not (
            out.is_contiguous(memory_format=torch.channels_last) if channels_last else out.is_contiguous()):
        raise ValueError(f"out must be a dense [N, 3, {shape[2]}, {shape[3]}] tensor on the GPU in the requested layout")
    return out


def _double3(values):
    return (ctypes.c_double * 3)(*[float(v) for v in values])


def image_normalize_pad(images, mean=None, std=None, to_rgb=False, size_divisor=32, dtype=torch.float16,
                        channels_last=False, out=None):
    """images [N, H0, W0, 3] uint8 or float32 on the GPU (BGR, as cv2 loads them) ->
    [N, 3, Hp, Wp] `dtype` (memory format channels_last if asked), normalised and zero padded."""
    assert images.is_cuda and images.dim() == 4 and images.shape[-1] == 3
    if images.dtype not in (torch.uint8, torch.float32):
        raise TypeError("images must be uint8 or float32")
    mean = IMG_NORM_CFG["mean"] if mean is None else mean
    std = IMG_NORM_CFG["std"] if std is None else std
    N, H0, W0, _ = images.shape
    Hp, Wp = padded_size(H0, W0, size_divisor)
    images = images.contiguous()
    out = _dense_out(out, (N, 3, Hp, Wp), dtype, images.device, channels_last, any_gpu=True)
    m, s = _double3(mean), _double3(std)
    handle = _lib.load_library()
    with torch.cuda.device(images.device):
        st = handle.bevops_image_normalize_pad(
            _lib.U8 if images.dtype == torch.uint8 else _lib.F32, images.data_ptr(), _lib.torch_dtype_code(out),
            out.data_ptr(), N, H0, W0, Hp, Wp, m, s, int(bool(to_rgb)), int(bool(channels_last)),
            _lib.current_stream_ptr(images.device))
    _lib.check(st, "bevops_image_normalize_pad")
    return out


# --------------------------------------------------------------------------- BEVFormer tiny / small: normalise + rescale + pad
# (csrc/image_scale.hip, design/image_scale.md): NormalizeMultiviewImage -> RandomScaleImageMultiViewImage -> Pad of the
# three shipped test pipelines (configs/bevformer/bevformer_tiny.py:19-20,229-231, bevformer_small.py:19,231-233,
# bevformer_base.py:11,228-231); scale None = the pipeline has no rescale step.
BEVFORMER_IMAGE_PIPELINES = {
    "tiny": dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True, scale=0.5, size_divisor=32),
    "small": dict(mean=[103.530, 116.280, 123.675], std=[1.0, 1.0, 1.0], to_rgb=False, scale=0.8, size_divisor=32),
    "base": dict(mean=[103.530, 116.280, 123.675], std=[1.0, 1.0, 1.0], to_rgb=False, scale=None, size_divisor=32),
}


def scaled_size(H0, W0, scale):
    """(height, width) RandomScaleImageMultiViewImage asks mmcv.imresize for (transform_3d.py:424-425): int(size * scale)
    in Python floats; scale None (no rescale step) leaves the size."""
    if scale is None:
        return int(H0), int(W0)
    return int(H0 * scale), int(W0 * scale)


def scale_lidar2img(lidar2img, scale):
    """diag(s, s, 1, 1) @ lidar2img in float64, then ONE rounding to float32 (transform_3d.py:426-433 followed by
    tools/bevformer/evaluate_trt.py:99,131-132) for [..., 4, 4] host or device tensors: rows 0 and 1 times `scale`.
    scale None returns the float32 cast alone."""
    m = torch.as_tensor(lidar2img).detach().to(torch.float64)
    if scale is not None:
        m = m.clone()
        m[..., :2, :] *= float(scale)
    return m.to(torch.float32)


def image_normalize_resize_pad(images, scale=None, size=None, mean=None, std=None, to_rgb=False, size_divisor=32,
                               dtype=torch.float16, channels_last=False, out=None):
    """images [N, H0, W0, 3] uint8 or float32 on the GPU (BGR, as cv2 loads them) -> normalised, resized to
    `size` = (Hs, Ws) or `scaled_size(H0, W0, scale)` with float32 bilinear interpolation in cv::resize's operation
    order (include/bevops.h), zero padded to multiples of `size_divisor`: [N, 3, Hp, Wp] `dtype` (memory format
    channels_last if asked).  One launch, no allocation when `out` is given.  Neither scale nor size: no resize, the
    result equals image_normalize_pad's bit for bit."""
    assert images.is_cuda and images.dim() == 4 and images.shape[-1] == 3
    if images.dtype not in (torch.uint8, torch.float32):
        raise TypeError("images must be uint8 or float32")
    if scale is not None and size is not None:
        raise ValueError("give scale or size, not both")
    mean = IMG_NORM_CFG["mean"] if mean is None else mean
    std = IMG_NORM_CFG["std"] if std is None else std
    N, H0, W0, _ = images.shape
    Hs, Ws = (int(size[0]), int(size[1])) if size is not None else scaled_size(H0, W0, scale)
    if Hs <= 0 or Ws <= 0:
        raise ValueError(f"the resized image would be {Hs} x {Ws}")
    Hp, Wp = padded_size(Hs, Ws, size_divisor)
    images = images.contiguous()
    out = _dense_out(out, (N, 3, Hp, Wp), dtype, images.device, channels_last, any_gpu=True)
    m, s = _double3(mean), _double3(std)
    handle = _lib.load_library()
    with torch.cuda.device(images.device):
        st = handle.bevops_image_normalize_resize_pad(
            _lib.U8 if images.dtype == torch.uint8 else _lib.F32, images.data_ptr(), _lib.torch_dtype_code(out),
            out.data_ptr(), N, H0, W0, Hs, Ws, Hp, Wp, m, s, int(bool(to_rgb)), int(bool(channels_last)),
            _lib.current_stream_ptr(images.device))
    _lib.check(st, "bevops_image_normalize_resize_pad")
    return out


# --------------------------------------------------------------------------- BEVDet: PIL-exact resize + crop + normalise
# (csrc/image_prepare.hip, design/image_prepare.md): what the test branch of the reference's PrepareImageInputs
# (third_party/bev_mmdet3d/datasets/pipelines/loading.py:691-792) computes, with the image work on the device.
BEVDET_IMG_NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)   # loading.py:694-696


def bevdet_test_augmentation(H, W, data_config, flip=None, scale=None):
    """The geometry BEVDet's test pipeline gives a raw H x W camera image (PrepareImageInputs.sample_augmentation with
    is_train=False) -> (resize, resize_dims (W, H), crop (x0, y0, x1, y1), flip, rotate = 0).  All in float64, each
    int() truncating: the resize ratio is the one that brings the width to the network's, plus `scale` (or the
    config's resize_test); the crop window has the network's size, is centred horizontally, and its lower edge lies
    where the mean of crop_h is cut off the bottom of the resized image."""
    net_h, net_w = data_config["input_size"]
    extra = data_config.get("resize_test", 0.0) if scale is None else scale
    resize = float(net_w) / float(W) + extra
    resized_w, resized_h = int(W * resize), int(H * resize)
    cut = data_config["crop_h"]
    lower_edge = int((1 - (cut[0] + cut[1]) / 2) * resized_h)
    x0 = int(max(0, resized_w - net_w) / 2)
    y0 = lower_edge - net_h
    return resize, (resized_w, resized_h), (x0, y0, x0 + net_w, y0 + net_h), bool(flip), 0


def bevdet_post_transform(resize, crop, flip):
    """The map from raw-image pixels to prepared-image pixels that this geometry implies, as BEVDet's view transformer
    takes it -> (post_rot [3, 3], post_tran [3]) float32: a scale by `resize`, a shift by the crop's corner and, when
    flipped, the mirror x -> crop width - x.  The values are those of PrepareImageInputs.img_transform at rotate = 0
    bit for bit (tests/golden/image_prepare.npz): float32(resize) on the diagonal, every zero a +0.0."""
    x0, y0, x1, y1 = (float(v) for v in crop)
    s = torch.tensor(float(resize), dtype=torch.float32)            # one rounding, to nearest
    post_rot, post_tran = torch.zeros(3, 3), torch.zeros(3)
    post_rot[0, 0], post_rot[1, 1], post_rot[2, 2] = s, s, 1.0
    post_tran[0], post_tran[1] = 0.0 - x0, 0.0 - y0                 # (0 - x, not -x: a zero offset stays +0.0)
    if flip:
        post_rot[0, 0] = -s
        post_tran[0] = (x1 - x0) - post_tran[0]
    return post_rot, post_tran


class ImageResizePlan:
    """Pillow's coefficient and bounds tables of one (source size, resize_dims, crop), built on the host by
    bevops_image_resize_plan_build (layout: include/bevops.h) and held on `device`."""
    HEADER = 16

    def __init__(self, H0, W0, resize_dims, crop, device):
        handle = _lib.load_library()
        self.H0, self.W0 = int(H0), int(W0)
        self.resize_dims = tuple(int(v) for v in resize_dims)
        self.crop = tuple(int(v) for v in crop)
        self.geometry = (self.H0, self.W0) + self.resize_dims + self.crop
        self.nbytes = handle.bevops_image_resize_plan_size(*self.geometry)
        if self.nbytes == 0:
            raise _lib.BevopsError(f"image_resize_plan: geometry {self.geometry} is outside the domain "
                                   "(include/bevops.h: crop inside the resized image, one tile's window within 64 KiB)",
                                   _lib.NOT_SUPPORTED)
        self.host = torch.empty(self.nbytes // 4, dtype=torch.int32)
        _lib.check(handle.bevops_image_resize_plan_build(*self.geometry, self.host.data_ptr(), self.nbytes),
                   "bevops_image_resize_plan_build")
        self.device = torch.device(device)
        self.tensor = self.host.to(self.device)
        self.out_size = (self.crop[3] - self.crop[1], self.crop[2] - self.crop[0])      # (fH, fW)

    def tables(self):
        """(bounds_x [fW, 2], coef_x [fW, ksize_x], bounds_y [fH, 2], coef_y [fH, ksize_y]) int32 host tensors."""
        fH, fW = self.out_size
        ksx, ksy = int(self.host[9]), int(self.host[10])
        sizes = (2 * fW, fW * ksx, 2 * fH, fH * ksy)
        bx, kx, by, ky = torch.split(self.host[self.HEADER:], sizes)
        return bx.view(fW, 2), kx.view(fW, ksx), by.view(fH, 2), ky.view(fH, ksy)


_PLANS = {}


def image_resize_plan(H0, W0, resize_dims, crop, device):
    """The cached device plan of one geometry: resize_dims = (W, H) and crop = (x0, y0, x1, y1) as
    `bevdet_test_augmentation` (PIL's conventions) gives them."""
    key = (int(H0), int(W0), tuple(int(v) for v in resize_dims), tuple(int(v) for v in crop), str(torch.device(device)))
    if key not in _PLANS:
        _PLANS[key] = ImageResizePlan(H0, W0, resize_dims, crop, device)
    return _PLANS[key]


def image_resize_crop_normalize(images, plan, flip=False, mean=None, std=None, to_rgb=True, dtype=torch.float16,
                                channels_last=False, out=None, canvas=None):
    """images [N, H0, W0, 3] uint8 RGB on the GPU -> [N, 3, fH, fW] `dtype`: img.resize(resize_dims).crop(crop), the
    optional left-right flip and mmlabNormalize, bit-exact to PIL, one launch, no allocation when `out` (and `canvas`)
    are given.  canvas: None -- not kept; True -- returned as a new [N, fH, fW, 3] uint8 tensor; a tensor -- filled.
    Returns `out`, or (out, canvas) when a canvas was asked for."""
    assert images.is_cuda and images.dim() == 4 and images.shape[-1] == 3
    if images.dtype != torch.uint8:
        raise TypeError("images must be uint8")
    mean = BEVDET_IMG_NORM["mean"] if mean is None else mean
    std = BEVDET_IMG_NORM["std"] if std is None else std
    N, H0, W0, _ = images.shape
    if (H0, W0) != (plan.H0, plan.W0) or plan.tensor.device != images.device:
        raise ValueError(f"the plan is for {plan.H0} x {plan.W0} images on {plan.tensor.device}")
    fH, fW = plan.out_size
    images = images.contiguous()
    out = _dense_out(out, (N, 3, fH, fW), dtype, images.device, channels_last)
    if canvas is True:
        canvas = torch.empty((N, fH, fW, 3), dtype=torch.uint8, device=images.device)
    elif canvas is not None and canvas is not False:
        if tuple(canvas.shape) != (N, fH, fW, 3) or canvas.dtype != torch.uint8 or canvas.device != images.device \
                or not canvas.is_contiguous():
            raise ValueError(f"canvas must be a dense [N, {fH}, {fW}, 3] uint8 tensor on the GPU")
    else:
        canvas = None
    m, s = _double3(mean), _double3(std)
    handle = _lib.load_library()
    with torch.cuda.device(images.device):
        st = handle.bevops_image_resize_crop_normalize(
            images.data_ptr(), plan.tensor.data_ptr(), plan.nbytes, _lib.torch_dtype_code(out), out.data_ptr(),
            None if canvas is None else canvas.data_ptr(), N, *plan.geometry, 0, m, s, int(bool(to_rgb)), int(bool(flip)),
            int(bool(channels_last)), _lib.current_stream_ptr(images.device))
    _lib.check(st, "bevops_image_resize_crop_normalize")
    return out if canvas is None else (out, canvas)


# --------------------------------------------------------------------------- 2-D detectors: keep-ratio resize + paste + normalise
# (csrc/image_letterbox.hip, design/letterbox.md): mmdet's test pipelines of the two 2-D detectors.  YOLOX
# (configs/yolox/yolox_x_8x8_300e_coco.py:75-92) resizes the uint8 image (arith 0: cv::resize's 8-bit fixed point), pads
# with 114 at the bottom / right and only casts; CenterNet (configs/centernet/centernet_resnet18_dcnv2_140e_coco.py:
# 38-41,69-110) resizes the float32 image (arith 1), pastes it CENTRED into a zero canvas and normalises last.
DETECT2D_IMAGE_PIPELINES = {
    "yolox": dict(arith=0, mean=[0.0, 0.0, 0.0], std=[1.0, 1.0, 1.0], to_rgb=False, pad=[114.0, 114.0, 114.0],
                  img_scale=(640, 640)),
    "centernet": dict(arith=1, mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True,
                      pad=[0.0, 0.0, 0.0], img_scale=(640, 640)),
}


def keep_ratio_size(H0, W0, img_scale=(640, 640)):
    """mmcv.rescale_size for a (long edge, short edge) bound -> (Hs, Ws): the largest factor that keeps the long side
    within max(img_scale) and the short side within min(img_scale), each size int(x * s + 0.5) in Python floats."""
    s = min(max(img_scale) / max(H0, W0), min(img_scale) / min(H0, W0))
    return int(H0 * s + 0.5), int(W0 * s + 0.5)


def _geometry(H0, W0, size, canvas, offset, **extra):
    (Hs, Ws), (Hp, Wp) = size, canvas
    scale = np.array([Ws / W0, Hs / H0, Ws / W0, Hs / H0], dtype=np.float32)       # mmcv.imresize(return_scale=True)
    return dict(ori_shape=(int(H0), int(W0), 3), img_shape=(Hs, Ws, 3), pad_shape=(Hp, Wp, 3), batch_input_shape=(Hp, Wp),
                size=(Hs, Ws), offset=(int(offset[0]), int(offset[1])), scale_factor=scale, **extra)


def yolox_test_geometry(H0, W0, img_scale=(640, 640)):
    """What YOLOX's test pipeline does to an H0 x W0 image: Resize(keep_ratio) to `size` = (Hs, Ws), the square
    max(Hs, Ws) canvas padded at the bottom / right (`offset` (0, 0)).  The dict is an img_metas entry that
    yolox_get_bboxes accepts as is (`scale_factor` float32 [w, h, w, h], `img_shape`, `pad_shape`)."""
    Hs, Ws = keep_ratio_size(H0, W0, img_scale)
    side = max(Hs, Ws)
    return _geometry(H0, W0, (Hs, Ws), (side, side), (0, 0))


def centernet_test_geometry(H0, W0, img_scale=(640, 640), pad_or=31, add_pix=1):
    """What CenterNet's test pipeline does to an H0 x W0 image: Resize(keep_ratio), RandomCenterCropPad(test_mode,
    ("logical_or", pad_or), add_pix): the resized image pasted CENTRED into a ((Hs | pad_or) + add_pix, (Ws | pad_or) +
    add_pix) canvas, `border` = float32 [top, bottom, left, right] of the paste, then Pad(pad_to_square) at the bottom /
    right.  The dict is an img_metas entry that centernet_get_bboxes accepts as is."""
    Hs, Ws = keep_ratio_size(H0, W0, img_scale)
    th, tw = (Hs | pad_or) + add_pix, (Ws | pad_or) + add_pix
    cy, cx = Hs // 2, Ws // 2
    top, bottom = cy - max(0, cy - th // 2), min(cy + th // 2, Hs) - cy
    left, right = cx - max(0, cx - tw // 2), min(cx + tw // 2, Ws) - cx
    oy, ox = th // 2 - top, tw // 2 - left
    border = np.array([oy, th // 2 + bottom, ox, tw // 2 + right], dtype=np.float32)
    side = max(th, tw)
    return _geometry(H0, W0, (Hs, Ws), (side, side), (oy, ox), border=border, crop_shape=(th, tw))


def image_letterbox(images, geometry, pipeline, dtype=torch.float16, channels_last=False, out=None):
    """images [N, H0, W0, 3] uint8 on the GPU (BGR, as cv2 loads them) -> [N, 3, Hp, Wp] `dtype` (memory format
    channels_last if asked): resized to geometry["size"], pasted at geometry["offset"] into the constant canvas
    geometry["pad_shape"], normalised -- one launch, no allocation when `out` is given.  geometry: yolox_test_geometry /
    centernet_test_geometry (or any dict with those three keys); pipeline: a name or an entry of
    DETECT2D_IMAGE_PIPELINES (arith, mean, std, to_rgb, pad; include/bevops.h: bevops_image_letterbox)."""
    assert images.is_cuda and images.dim() == 4 and images.shape[-1] == 3
    if images.dtype != torch.uint8:
        raise TypeError("images must be uint8")
    p = DETECT2D_IMAGE_PIPELINES[pipeline] if isinstance(pipeline, str) else pipeline
    N, H0, W0, _ = images.shape
    if "ori_shape" in geometry and tuple(geometry["ori_shape"][:2]) != (H0, W0):
        raise ValueError(f"the geometry is for {tuple(geometry['ori_shape'][:2])} images, got {(H0, W0)}")
    (Hs, Ws), (Hp, Wp), (oy, ox) = geometry["size"], geometry["pad_shape"][:2], geometry["offset"]
    images = images.contiguous()
    out = _dense_out(out, (N, 3, Hp, Wp), dtype, images.device, channels_last)
    pad, m, s = _double3(p["pad"]), _double3(p["mean"]), _double3(p["std"])
    handle = _lib.load_library()
    with torch.cuda.device(images.device):
        st = handle.bevops_image_letterbox(
            int(p["arith"]), images.data_ptr(), _lib.torch_dtype_code(out), out.data_ptr(), N, H0, W0, int(Hs), int(Ws),
            int(Hp), int(Wp), int(oy), int(ox), pad, m, s, int(bool(p["to_rgb"])), int(bool(channels_last)),
            _lib.current_stream_ptr(images.device))
    _lib.check(st, "bevops_image_letterbox")
    return out
