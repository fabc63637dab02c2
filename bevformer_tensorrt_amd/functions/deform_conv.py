"""deform_conv2d / deform_conv2d_nhwc -- the UNMODULATED deformable convolution (DCNv1: mmcv.ops.deform_conv2d) that
mmcv's `DCN` pack runs in BEVDepth's DepthNet (third_party/bev_mmdet3d/models/necks/view_transformer.py:590-601).  Not
a reference plugin.  design/bevdepth_dcn.md.

  deform_conv2d_nhwc  the fast path: channels-last fp16, 3 x 3 / stride 1 / pad 1, one deform group, any number of conv
                      groups in ONE launch (bevops_deform_conv3x3_nhwc_f16), offsets straight from conv_offset_nhwc;
  deform_conv2d_q_nhwc  its INT8 form on int8 channel slices (bevops_deform_conv3x3_nhwc_s8): fp16 offsets, the sampled
                      column rounded to int8 in the INPUT's scale, exact int32 sums (design/bevdepth_dcn_int8.md);
  deform_conv2d       the plain path in mmcv's argument order on NCHW tensors: on CUDA the package's DCNv2 operator with
                      a mask of ones, on CPU a torch statement of the same sampling rules."""
import torch
from torch.nn.modules.utils import _pair

from ..utils import lib as _lib
from . import yolox_ops as _Y
from .modulated_deformable_conv2d import _PACKED, _packed_weight, modulated_deformable_conv2d


def deform_conv_packed_weight(weight, build=True):
    """The [Cout][tap][Cin / groups] image of an fp16 CUDA weight [Cout, Cin / groups, 3, 3]
    (bevops_mdconv_pack_weight), cached per weight tensor and version in the cache modulated_deformable_conv2d_nhwc
    uses.  build=False: None when it is missing or stale.  Never made under stream capture (RuntimeError)."""
    hit = _PACKED.get(weight)
    if hit is not None or not build:
        return hit
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("deform_conv2d_nhwc: the packed weight is missing or stale and the stream is capturing; call "
                           "BEVDet.prepare_bev_half() (or the operator once, eagerly) before the capture")
    return _packed_weight(_lib.load_library(), weight, _lib.F16)


def deform_conv2d_nhwc(input, offset_nhwc, weight, bias=None, groups=1, relu=False):
    """input [B, Cin, H, W] fp16 CUDA in torch.channels_last; offset_nhwc [B, OC >= 18, H, W] channels-last, the raw
    output of the pack's offset convolution (conv_offset_nhwc: OC = 32; channels >= 18 are never read); weight
    [Cout, Cin / groups, 3, 3] fp16 contiguous; bias [Cout] fp16 or None -> [B, Cout, H, W] channels-last.  Domain:
    (Cin / groups) % 32 == 0 and (Cout / groups) % 32 == 0 (BevopsError, status 3, otherwise)."""
    for name, t in (("input", input), ("offset_nhwc", offset_nhwc), ("weight", weight)):
        if not (t.is_cuda and t.dtype == torch.float16 and t.dim() == 4):
            raise TypeError(f"deform_conv2d_nhwc: {name} must be a 4-D fp16 CUDA tensor")
    if not input.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("deform_conv2d_nhwc: input must be in torch.channels_last")
    if not offset_nhwc.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("deform_conv2d_nhwc: offset_nhwc must be in torch.channels_last")
    if not weight.is_contiguous():
        raise ValueError("deform_conv2d_nhwc: weight must be contiguous")
    B, Cin, H, W = input.shape
    Cout, cin_g, Kh, Kw = weight.shape
    if (Kh, Kw) != (3, 3) or groups <= 0 or cin_g * groups != Cin:
        raise ValueError(f"deform_conv2d_nhwc: weight {tuple(weight.shape)} does not fit {Cin} input channels in {groups} "
                         "groups of a 3 x 3 kernel")
    OC = offset_nhwc.shape[1]
    if (offset_nhwc.shape[0], offset_nhwc.shape[2], offset_nhwc.shape[3]) != (B, H, W):
        raise ValueError(f"deform_conv2d_nhwc: offset_nhwc {tuple(offset_nhwc.shape)} does not cover input {tuple(input.shape)}")
    if bias is not None and not (bias.is_cuda and bias.dtype == torch.float16 and bias.is_contiguous() and bias.shape == (Cout,)):
        raise ValueError("deform_conv2d_nhwc: bias must be a contiguous fp16 CUDA tensor [Cout]")
    packed = deform_conv_packed_weight(weight)
    out = torch.empty((B, Cout, H, W), dtype=input.dtype, device=input.device, memory_format=torch.channels_last)
    if B == 0:
        return out
    handle = _lib.load_library()
    with torch.cuda.device(input.device):
        st = handle.bevops_deform_conv3x3_nhwc_f16(input.data_ptr(), offset_nhwc.data_ptr(), OC, packed.data_ptr(),
                                                   bias.data_ptr() if bias is not None else None, out.data_ptr(),
                                                   int(bool(relu)), B, H, W, Cin, Cout, groups,
                                                   _lib.current_stream_ptr(input.device))
    _lib.check(st, "bevops_deform_conv3x3_nhwc_f16")
    return out


def deform_conv2d_q_nhwc(x_q, scale_x, offset_nhwc, w_q_taps, w_scales, bias, groups, out=None, scale_out=None,
                         out_dtype=torch.int8, relu=False):
    """bevops_deform_conv3x3_nhwc_s8: the grouped, unmodulated deformable 3 x 3 convolution (stride 1, padding 1, one
    deform group) of an int8 channel slice x_q [B, Cin, H, W] (real = q scale_x) with int8 taps-major weights w_q_taps
    [Cout, 3, 3, Cin / groups] (real = q w_scales[co]: yolox_ops.quantize_weight_taps of [Cout, Cin / groups, 3, 3]);
    offset_nhwc [B, OC >= 18, H, W] fp16 channels-last (or a channel slice), the raw rows of the offset convolution,
    NOT quantised; w_scales / bias fp32 [Cout] or None.  out_dtype torch.int8: requantised with scale_out;
    torch.float16: one rounding.  x_q and out may be channel slices of wider buffers.  Domain: (Cin / groups) % 32 == 0
    and (Cout / groups) % 32 == 0 (BevopsError NOT_SUPPORTED otherwise).  Nothing is packed: no capture guard.
    include/bevops.h states the operation order."""
    if not (x_q.is_cuda and x_q.dtype == torch.int8):
        raise TypeError("deform_conv2d_q_nhwc: x_q must be an int8 CUDA tensor")
    if not (offset_nhwc.is_cuda and offset_nhwc.dtype == torch.float16 and offset_nhwc.dim() == 4 and
            offset_nhwc.device == x_q.device):
        raise TypeError("deform_conv2d_q_nhwc: offset_nhwc must be a 4-D fp16 CUDA tensor on the input's device")
    if w_q_taps.dim() != 4 or tuple(w_q_taps.shape[1:3]) != (3, 3) or not w_q_taps.is_contiguous() or \
            w_q_taps.dtype != torch.int8 or w_q_taps.device != x_q.device:
        raise ValueError("deform_conv2d_q_nhwc: w_q_taps [Cout, 3, 3, Cin / groups] contiguous int8 on the input's device")
    xp = _Y.slice_pitch(x_q, "x_q")
    B, Cin, H, W = x_q.shape
    Cout, cin_g = w_q_taps.shape[0], w_q_taps.shape[3]
    groups = int(groups)
    if groups <= 0 or cin_g * groups != Cin or Cout % groups:
        raise ValueError(f"deform_conv2d_q_nhwc: weight {tuple(w_q_taps.shape)} does not fit {Cin} input channels in "
                         f"{groups} groups of a 3 x 3 kernel")
    if (offset_nhwc.shape[0], offset_nhwc.shape[2], offset_nhwc.shape[3]) != (B, H, W):
        raise ValueError(f"deform_conv2d_q_nhwc: offset_nhwc {tuple(offset_nhwc.shape)} does not cover input "
                         f"{tuple(x_q.shape)}")
    # the entry reads rows of OC channels: the tensor's own in torch.channels_last, else the pitch of a channel slice
    OC = offset_nhwc.shape[1] if offset_nhwc.is_contiguous(memory_format=torch.channels_last) else \
        _Y.slice_pitch(offset_nhwc, "offset_nhwc")
    if offset_nhwc.shape[1] < 18 or OC % 2 or offset_nhwc.data_ptr() % 16:
        raise ValueError("deform_conv2d_q_nhwc: offset_nhwc has at least 18 channels, an even row pitch and a 16-byte "
                         "aligned start")
    if out_dtype not in (torch.int8, torch.float16):
        raise ValueError("deform_conv2d_q_nhwc: out_dtype torch.int8 or torch.float16")
    if out is not None and out.dtype != out_dtype:
        raise ValueError(f"deform_conv2d_q_nhwc: out is {out.dtype}, out_dtype {out_dtype}")
    out8 = out_dtype == torch.int8
    if cin_g % 32 or (Cout // groups) % 32:
        raise _lib.BevopsError("bevops_deform_conv3x3_nhwc_s8: (Cin / groups) % 32 == 0 and (Cout / groups) % 32 == 0",
                               _lib.NOT_SUPPORTED)
    sx = _Y._scale(scale_x, "scale_x")
    so = _Y._scale(scale_out, "scale_out") if out8 else 1.0
    for t, name in ((w_scales, "w_scales"), (bias, "bias")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != Cout or
                              t.device != x_q.device):
            raise ValueError(f"deform_conv2d_q_nhwc: {name} contiguous fp32 [Cout] on the input's device")
    if out is None:
        out = _Y.nhwc_empty(B, Cout, H, W, x_q.device, out_dtype)
    elif tuple(out.shape) != (B, Cout, H, W) or out.device != x_q.device:
        raise ValueError(f"deform_conv2d_q_nhwc: out must be {(B, Cout, H, W)} on {x_q.device}, got {tuple(out.shape)}")
    op = _Y.slice_pitch(out, "out")
    if B == 0:
        return out
    handle = _lib.load_library()
    with torch.cuda.device(x_q.device):
        st = handle.bevops_deform_conv3x3_nhwc_s8(x_q.data_ptr(), xp, sx, offset_nhwc.data_ptr(), OC, w_q_taps.data_ptr(),
                                                  None if w_scales is None else w_scales.data_ptr(), 1.0,
                                                  None if bias is None else bias.data_ptr(),
                                                  _lib.I8 if out8 else _lib.F16, out.data_ptr(), op, so, int(bool(relu)),
                                                  B, H, W, Cin, Cout, groups, _lib.current_stream_ptr(x_q.device))
    _lib.check(st, "bevops_deform_conv3x3_nhwc_s8")
    return out


def _deform_conv2d_cpu(input, offset, weight, stride, padding, dilation, groups, deform_groups, column=None):
    """The torch statement: positions h = ho * stride - pad + i * dil + off_h (w likewise), a tap is live iff
    -1 < h < H and -1 < w < W, bilinear with the corners outside the image contributing zero; then the grouped product
    with the weights.  In the input's dtype, on the input's device.  column: a function applied to the sampled column
    [B, Cin, K * K, Ho, Wo] in front of the product (the INT8 statement rounds it there); None: nothing."""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    B, Cin, H, W = input.shape
    Cout, cin_g, Kh, Kw = weight.shape
    kk = Kh * Kw
    Ho = (H + 2 * ph - (dh * (Kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (Kw - 1) + 1)) // sw + 1
    if tuple(offset.shape) != (B, deform_groups * 2 * kk, Ho, Wo):
        raise ValueError(f"offset shape {tuple(offset.shape)} != {(B, deform_groups * 2 * kk, Ho, Wo)}")
    if cin_g * groups != Cin or Cout % groups or Cin % deform_groups:
        raise ValueError("deform_conv2d: channels do not divide into the groups")
    dt = input.dtype
    offset, weight = offset.to(dt), weight.to(dt)
    cpd = Cin // deform_groups
    dev = input.device
    base_h = (torch.arange(Ho, dtype=dt, device=dev) * sh - ph).view(1, Ho, 1)
    base_w = (torch.arange(Wo, dtype=dt, device=dev) * sw - pw).view(1, 1, Wo)
    flat = input.reshape(B, Cin, H * W)
    zero = torch.zeros((), dtype=dt, device=dev)
    cols = []
    for dg in range(deform_groups):
        xg = flat[:, dg * cpd:(dg + 1) * cpd]
        taps = []
        for tap in range(kk):
            i, j = divmod(tap, Kw)
            h = base_h + i * dh + offset[:, (dg * kk + tap) * 2]
            w = base_w + j * dw + offset[:, (dg * kk + tap) * 2 + 1]
            live = (h > -1) & (h < H) & (w > -1) & (w < W)
            h0, w0 = torch.floor(h), torch.floor(w)
            lh, lw = h - h0, w - w0
            acc = None
            for a, b, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
                hc, wc = h0 + a, w0 + b
                inside = live & (hc >= 0) & (hc <= H - 1) & (wc >= 0) & (wc <= W - 1)
                idx = (hc.clamp(0, H - 1) * W + wc.clamp(0, W - 1)).long().view(B, 1, Ho * Wo).expand(B, cpd, Ho * Wo)
                v = torch.gather(xg, 2, idx).view(B, cpd, Ho, Wo)
                term = torch.where(inside.unsqueeze(1), wt.unsqueeze(1) * v, zero)
                acc = term if acc is None else acc + term
            taps.append(acc)
        cols.append(torch.stack(taps, dim=2))                                        # [B, cpd, kk, Ho, Wo]
    col = torch.cat(cols, dim=1) if deform_groups > 1 else cols[0]
    if column is not None:
        col = column(col)
    cout_g = Cout // groups
    out = torch.empty(B, Cout, Ho, Wo, dtype=dt, device=dev)
    for g in range(groups):
        wg = weight[g * cout_g:(g + 1) * cout_g].reshape(cout_g, cin_g * kk)         # k = (ci, tap)
        cg = col[:, g * cin_g:(g + 1) * cin_g].reshape(B, cin_g * kk, Ho * Wo)
        out[:, g * cout_g:(g + 1) * cout_g] = torch.matmul(wg.unsqueeze(0), cg).view(B, cout_g, Ho, Wo)
    return out


def deform_conv2d(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deform_groups=1):
    """mmcv.ops.deform_conv2d's forward (no bias, as there): input [B, Cin, H, W], offset [B, dg * 2 * K * K, Ho, Wo]
    ((h, w) per tap, taps row-major), weight [Cout, Cin / groups, K, K].  CUDA fp16 / fp32: the package's DCNv2 operator
    with a mask of ones.  CPU: the torch statement above, in the input's dtype."""
    if input.dim() != 4:
        raise ValueError(f"Expected 4D tensor as input, got {input.dim()}D tensor instead.")
    if input.is_cuda:
        Kh, Kw = weight.shape[2:]
        ones = torch.ones((offset.shape[0], deform_groups * Kh * Kw) + tuple(offset.shape[2:]), dtype=offset.dtype,
                          device=offset.device)
        return modulated_deformable_conv2d(input, offset, ones, weight, None, stride, padding, dilation, groups,
                                           deform_groups)
    return _deform_conv2d_cpu(input, offset, weight, stride, padding, dilation, groups, deform_groups)
