"""The layers of YOLOX (bevformer_tensorrt_amd/yolox.py) on CHANNEL SLICES of channels-last fp16 tensors: the
convolution with SiLU / ReLU and the identity behind the activation (bevops_conv_slice_f16, csrc/conv_slice.hip), Focus,
SPPBottleneck's three max-pools and nearest 2 x up-sampling (csrc/yolox.hip).  Not reference plugins (TensorRT owns
these layers there).

A channel slice is a [B, C, H, W] view `buf[:, c0:c0 + C]` of a channels-last tensor `buf` [B, Ct, H, W]: strides
(H W Ct, 1, W Ct, Ct).  Ct is the slice's PITCH.  Every function here reads slices through their pitch and, with
`out=`, writes into a slice: the producers of a concatenated tensor write their shares of ONE buffer and nobody
copies.  A slice starts on a 16-byte boundary (c0 % 8 == 0) and its pitch is a multiple of 8.

Channel padding: the convolution kernel needs Cin % 32 == 0.  A layer of other width (YOLOX-x's 80-channel layers) runs
at the next multiple of 32 with zero weight rows and columns and zero bias: `pad_channels`.  A pad channel is
act(0 + 0) + 0 = 0 exactly, for every activation here, so it stays zero through the network.

The INT8 flavours (the INT8 build of YOLOX, yolox_int8.py) live beside them: `conv_slice_q_taps`
(bevops_conv_slice_s8, csrc/conv_slice_s8.hip), `focus_nhwc_q`, and `spp_maxpool_nhwc` / `upsample_nearest2x_nhwc`
routed by dtype; an int8 slice's pitch is a multiple of 16 and c0 % 16 == 0.  `quantize_weight_taps` is their weight
quantiser."""
import torch

from ..utils import lib as _lib
from .linear import _call, _ptr
from .multi_scale_deformable_attn import _TensorCache

ACTS = {None: 0, "none": 0, "relu": 1, "silu": 2}
CHANNEL_MULTIPLE = 32
_PACKED = _TensorCache()   # weight tensor -> {(cin, cout): (taps-major padded weight)} (stamped as conv.pack_taps')


def padded_width(c, multiple=CHANNEL_MULTIPLE):
    return (int(c) + multiple - 1) // multiple * multiple


def _group_index(groups, multiple):
    """For channel groups of the given sizes, each padded to `multiple`: (index of every real channel in the padded
    axis, padded length)."""
    idx, at = [], 0
    for g in groups:
        idx += list(range(at, at + g))
        at += padded_width(g, multiple)
    return idx, at


def pad_channels(weight, bias=None, groups_in=None, groups_out=None, multiple=CHANNEL_MULTIPLE):
    """weight [Cout, Cin, k, k] (and bias [Cout]) with each channel group padded with zeros to a multiple of `multiple`.
    groups_in / groups_out: the sizes of the groups the input / output channels consist of (None: one group; a layer
    behind a concatenation of two padded 80-channel tensors has groups_in (80, 80) -> 192 input channels with the real
    ones at 0 .. 79 and 96 .. 175).  -> (padded weight, padded bias or None).  `unpad_channels` is the inverse."""
    cout, cin = weight.shape[:2]
    groups_in = (cin,) if groups_in is None else tuple(groups_in)
    groups_out = (cout,) if groups_out is None else tuple(groups_out)
    if sum(groups_in) != cin or sum(groups_out) != cout:
        raise ValueError("pad_channels: the groups must add up to the weight's channels")
    ii, pin = _group_index(groups_in, multiple)
    oi, pout = _group_index(groups_out, multiple)
    w = weight.detach()
    wp = w.new_zeros((pout, pin) + tuple(w.shape[2:]))
    ii_t, oi_t = torch.tensor(ii, device=w.device), torch.tensor(oi, device=w.device)
    wp[oi_t[:, None], ii_t[None, :]] = w
    bp = None
    if bias is not None:
        bp = bias.detach().new_zeros((pout,))
        bp[oi_t] = bias.detach()
    return wp, bp


def unpad_channels(weight, bias=None, groups_in=None, groups_out=None, multiple=CHANNEL_MULTIPLE):
    """The inverse of `pad_channels`: the real rows and columns of a padded weight (and bias); groups_* as there (the
    UNPADDED sizes)."""
    ii, pin = _group_index(groups_in, multiple)
    oi, pout = _group_index(groups_out, multiple)
    if tuple(weight.shape[:2]) != (pout, pin):
        raise ValueError("unpad_channels: the weight is not the padded form of these groups")
    ii_t, oi_t = torch.tensor(ii, device=weight.device), torch.tensor(oi, device=weight.device)
    w = weight[oi_t[:, None], ii_t[None, :]]
    return w, (None if bias is None else bias[oi_t])


def nhwc_empty(B, C, H, W, device, dtype=torch.float16):
    """An uninitialised channels-last tensor [B, C, H, W] with explicit strides (H W C, 1, W C, C) for every size,
    1 x 1 maps included: the buffer concatenated tensors are written into slice by slice."""
    return torch.empty((B, H, W, C), device=device, dtype=dtype).permute(0, 3, 1, 2)


def slice_pitch(t, name="tensor"):
    """The pitch (elements between two pixels) of a channel slice of a channels-last tensor, its layout and alignment
    checked: ValueError for anything else."""
    if t.dim() != 4:
        raise ValueError(f"{name}: a [B, C, H, W] tensor")
    B, C, H, W = t.shape
    if W > 1:
        pitch = t.stride(3)
    elif H > 1:
        pitch = t.stride(2)
    elif B > 1:
        pitch = t.stride(0)
    else:
        pitch = padded_width(C, 16 // t.element_size())
    ok = pitch >= C and (C == 1 or t.stride(1) == 1) and (W == 1 or t.stride(3) == pitch) and \
        (H == 1 or t.stride(2) == W * pitch) and (B == 1 or t.stride(0) == H * W * pitch)
    if not ok:
        raise ValueError(f"{name}: not a channel slice of a channels-last tensor (shape {tuple(t.shape)}, strides "
                         f"{tuple(t.stride())})")
    vec = 16 // t.element_size()               # elements per 16-byte vector: 8 (fp16), 16 (int8)
    if pitch % vec or t.data_ptr() % 16:
        raise ValueError(f"{name}: a slice starts on a 16-byte boundary and its pitch is a multiple of {vec} elements "
                         f"(pitch {pitch}, address % 16 = {t.data_ptr() % 16})")
    return pitch


def _check_f16(t, name):
    if not (t.is_cuda and t.dtype == torch.float16):
        raise ValueError(f"{name}: an fp16 CUDA tensor")


def _dest(out, shape, like, name):
    if out is None:
        return nhwc_empty(*shape, like.device, like.dtype)
    if tuple(out.shape) != tuple(shape) or out.dtype != like.dtype or out.device != like.device:
        raise ValueError(f"{name}: out must be {tuple(shape)} {like.dtype} on {like.device}, got {tuple(out.shape)}")
    return out


def conv_slice_packed_weight(weight, cin=None, cout=None, build=True):
    """The taps-major [cout, k, k, cin] operand of bevops_conv_slice_f16 for `weight` [Cout, Cin, k, k], zero-padded
    behind its rows / columns to cout / cin channels; cached per weight tensor with the stamp functions.conv.pack_taps
    uses and rebuilt when the weight changes.  build=False: None when missing or stale.  Never built inside a stream
    capture (RuntimeError)."""
    cout = weight.shape[0] if cout is None else int(cout)
    cin = weight.shape[1] if cin is None else int(cin)
    hit = _PACKED.get(weight)
    if hit is not None and (cin, cout) in hit:
        return hit[(cin, cout)]
    if not build:
        return None
    if weight.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("conv_slice_nhwc: the packed weight is missing or stale and the stream is capturing; call "
                           "conv_slice_packed_weight(weight, cin, cout) (or the layer once, eagerly) before the capture")
    if cout < weight.shape[0] or cin < weight.shape[1]:
        raise ValueError("conv_slice_nhwc: fewer channels than the weight has")
    w = weight.detach()
    wp = w.new_zeros((cout, w.shape[2], w.shape[3], cin))
    wp[:w.shape[0], :, :, :w.shape[1]] = w.permute(0, 2, 3, 1)
    if hit is None:
        hit = _PACKED.put(weight, {})
    hit[(cin, cout)] = wp
    return wp


def conv_slice_taps(x, weight_taps, bias=None, act="silu", residual=None, stride=1, out=None, dilation=1,
                    image_bias=None):
    """`conv_slice_nhwc` on an operand that already is taps-major: weight_taps [Cout, k, k, Cin] contiguous fp16 with
    Cin == x.shape[1] (callers that merge or pad their weights themselves: yolox.py).  dilation / image_bias as there
    (image_bias [B, P] fp16 with P >= Cout, P % 8 == 0, rows contiguous; it replaces `bias`)."""
    _check_f16(x, "x")
    if weight_taps.dim() != 4 or weight_taps.shape[1] != weight_taps.shape[2] or not weight_taps.is_contiguous() or \
            weight_taps.dtype != torch.float16 or weight_taps.device != x.device:
        raise ValueError("conv_slice: weight_taps [Cout, k, k, Cin] contiguous fp16 on the input's device")
    B, Cin, H, W = x.shape
    Cout, k = weight_taps.shape[0], weight_taps.shape[1]
    if weight_taps.shape[3] != Cin:
        raise ValueError(f"conv_slice: the weight has {weight_taps.shape[3]} input channels, x has {Cin}")
    if act not in ACTS:
        raise ValueError(f"conv_slice: act in {sorted(k for k in ACTS if k)}")
    if k not in (1, 3) or stride not in (1, 2) or Cin % 32 or Cout % 8:
        raise _lib.BevopsError("bevops_conv_slice_f16: ksize in {1, 3}, stride in {1, 2}, Cin % 32 == 0, Cout % 8 == 0",
                               _lib.NOT_SUPPORTED)
    dilation = int(dilation)
    if dilation < 1:
        raise ValueError("conv_slice: dilation >= 1")
    if dilation > 1 and (k != 3 or stride != 1):
        raise _lib.BevopsError("bevops_conv_slice_f16_ex: dilation > 1 needs ksize 3 and stride 1", _lib.NOT_SUPPORTED)
    bp = 0
    if image_bias is not None:
        if bias is not None:
            raise ValueError("conv_slice: image_bias replaces bias, pass one of them")
        _check_f16(image_bias, "image_bias")
        if image_bias.dim() != 2 or image_bias.shape[0] != B or image_bias.shape[1] < Cout or \
                (image_bias.shape[1] > 1 and image_bias.stride(1) != 1):
            raise ValueError(f"conv_slice: image_bias [B, >= Cout] with contiguous rows, got {tuple(image_bias.shape)}")
        bp = image_bias.stride(0) if B > 1 else padded_width(image_bias.shape[1], 8)
        if bp < Cout or bp % 8 or image_bias.data_ptr() % 16:
            raise ValueError(f"conv_slice: image_bias rows start on 16-byte boundaries, pitch a multiple of 8 (pitch {bp})")
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    xp = slice_pitch(x, "x")
    out = _dest(out, (B, Cout, Ho, Wo), x, "conv_slice")
    op = slice_pitch(out, "out")
    rp = 0
    if residual is not None:
        _check_f16(residual, "residual")
        if tuple(residual.shape) != tuple(out.shape):
            raise ValueError("conv_slice: the identity has the output's shape")
        rp = slice_pitch(residual, "residual")
    if bias is not None:
        if bias.numel() != Cout:
            raise ValueError("conv_slice: one bias per output channel")
        if bias.dtype != torch.float16 or not bias.is_contiguous():
            bias = bias.to(torch.float16).contiguous()
    if B == 0:
        return out
    if dilation == 1 and image_bias is None:
        _call("bevops_conv_slice_f16", x.device, x.data_ptr(), xp, weight_taps.data_ptr(), _ptr(bias), _ptr(residual), rp,
              out.data_ptr(), op, B, H, W, Cin, Cout, k, int(stride), ACTS[act])
    else:
        _call("bevops_conv_slice_f16_ex", x.device, x.data_ptr(), xp, weight_taps.data_ptr(),
              _ptr(bias if image_bias is None else image_bias), _ptr(residual), rp, out.data_ptr(), op, B, H, W, Cin, Cout,
              k, int(stride), ACTS[act], dilation, bp)
    return out


def conv_slice_nhwc(x, weight, bias=None, act="silu", residual=None, stride=1, out=None, dilation=1, image_bias=None):
    """out = act(conv2d(x, weight, stride, pad dilation * (k // 2), dilation) + bias) + residual, the identity AFTER the
    activation.  dilation > 1: k == 3 and stride == 1 (else BevopsError NOT_SUPPORTED).  image_bias [B, P] fp16 (P >= the
    output slice's channels, P % 8 == 0): a bias per IMAGE in place of `bias` -- output pixel (b, y, x) takes
    image_bias[b, co] (ASPP's pooled branch folded through its 1 x 1 convolution, design/bevdepth.md).
    x [B, Cx, H, W], residual and out [B, Co, Hout, Wout]: fp16 channel slices of channels-last tensors; weight
    [Cout, Cin, k, k] fp16 with k in {1, 3}; stride in {1, 2}; act in "none", "relu", "silu".  Cx >= Cin and, with
    `out=`, Co >= Cout: the layer runs at the tensors' widths with zero weight columns / rows (and zero bias) behind
    the weight's own -- an 80-channel layer on 96-channel tensors.  Without `out=` a new channels-last tensor of
    padded_width(Cout, 8) channels is returned.  Cx % 32 == 0, Co % 8 == 0 (else BevopsError NOT_SUPPORTED)."""
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise ValueError("conv_slice_nhwc: weight [Cout, Cin, k, k]")
    if weight.dtype != torch.float16 or weight.device != x.device:
        raise ValueError("conv_slice_nhwc: an fp16 weight on the input's device")
    cin = x.shape[1]
    cout = out.shape[1] if out is not None else padded_width(weight.shape[0], 8)
    if cin < weight.shape[1] or cout < weight.shape[0]:
        raise ValueError("conv_slice_nhwc: the tensors have fewer channels than the weight")
    if cin % 32 or cout % 8:
        raise _lib.BevopsError("bevops_conv_slice_f16: Cin % 32 == 0 and Cout % 8 == 0", _lib.NOT_SUPPORTED)
    wp = conv_slice_packed_weight(weight, cin, cout)
    if bias is not None and bias.numel() != cout:
        b = bias.detach().new_zeros((cout,))
        b[:bias.numel()] = bias.detach()
        bias = b
    if image_bias is not None and image_bias.dim() == 2 and image_bias.shape[1] < cout:
        raise ValueError("conv_slice_nhwc: image_bias has fewer columns than the output slice has channels")
    return conv_slice_taps(x, wp, bias, act, residual, stride, out, dilation, image_bias)


FOCUS_CHANNELS = 32


def focus_nhwc(image, out=None):
    """mmdet's Focus (space to depth) from the planar image: image [B, 3, H, W] contiguous fp16, H and W even -> a
    channel slice [B, 32, H/2, W/2]: channels 0 .. 11 = cat(top-left, bottom-left, top-right, bottom-right) patches of
    three channels each, channels 12 .. 31 zero (the stem convolution's Cin % 32 == 0)."""
    _check_f16(image, "image")
    if image.dim() != 4 or image.shape[1] != 3 or not image.is_contiguous():
        raise ValueError("focus_nhwc: a contiguous [B, 3, H, W] image")
    B, _, H, W = image.shape
    if H % 2 or W % 2:
        raise _lib.BevopsError("bevops_focus_nhwc: H and W even", _lib.NOT_SUPPORTED)
    out = _dest(out, (B, FOCUS_CHANNELS, H // 2, W // 2), image, "focus_nhwc")
    op = slice_pitch(out, "out")
    if B:
        _call("bevops_focus_nhwc", image.device, image.data_ptr(), out.data_ptr(), op, B, H, W)
    return out


def spp_maxpool_nhwc(x, out=None, kernel_sizes=(5, 9, 13)):
    """SPPBottleneck's pools: x a channel slice [B, C, H, W] -> a slice [B, 3 C, H, W] holding max_pool2d(x, k, stride
    1, padding k // 2) for the three odd k <= 13 behind each other.  x and out may be slices of one [B, 4 C, H, W]
    buffer (x = buf[:, :C], out = buf[:, C:]): the concatenation is then free.  One launch.  A NaN reaches every window
    that holds it, as in F.max_pool2d.  An int8 slice goes to bevops_spp_maxpool_nhwc_s8 (C % 16 == 0, padding -128;
    exact, the output keeps the input's scale)."""
    if x.dtype == torch.int8:
        return _spp_maxpool_s8(x, out, kernel_sizes)
    _check_f16(x, "x")
    B, C, H, W = x.shape
    ks = tuple(int(k) for k in kernel_sizes)
    if len(ks) != 3:
        raise ValueError("spp_maxpool_nhwc: three kernel sizes")
    if C % 8 or any(k % 2 == 0 or k > 13 or k < 1 for k in ks):
        raise _lib.BevopsError("bevops_spp_maxpool_nhwc: C % 8 == 0, odd kernel sizes <= 13", _lib.NOT_SUPPORTED)
    xp = slice_pitch(x, "x")
    out = _dest(out, (B, 3 * C, H, W), x, "spp_maxpool_nhwc")
    op = slice_pitch(out, "out")
    if B:
        _call("bevops_spp_maxpool_nhwc", x.device, x.data_ptr(), xp, out.data_ptr(), op, B, H, W, C, *ks)
    return out


def upsample_nearest2x_nhwc(x, out=None):
    """x a channel slice [B, C, H, W] -> a slice [B, C, 2H, 2W] = F.interpolate(x, scale_factor=2, mode="nearest").
    An int8 slice goes to bevops_upsample_nearest2x_nhwc_s8 (C % 16 == 0; a byte copy, the scale is the input's)."""
    s8 = x.dtype == torch.int8
    if s8:
        _check_s8(x, "x")
    else:
        _check_f16(x, "x")
    entry, vec = ("bevops_upsample_nearest2x_nhwc_s8", 16) if s8 else ("bevops_upsample_nearest2x_nhwc", 8)
    B, C, H, W = x.shape
    if C % vec:
        raise _lib.BevopsError(f"{entry}: C % {vec} == 0", _lib.NOT_SUPPORTED)
    xp = slice_pitch(x, "x")
    out = _dest(out, (B, C, 2 * H, 2 * W), x, "upsample_nearest2x_nhwc")
    op = slice_pitch(out, "out")
    if B:
        _call(entry, x.device, x.data_ptr(), xp, out.data_ptr(), op, B, H, W, C)
    return out


# ---- the INT8 flavours (the INT8 build of YOLOX, quantization.build_int8_yolox).  An int8 slice starts on a 16-byte
# boundary and its pitch is a multiple of 16; a tensor carries no scale: the caller passes it.

def _check_s8(t, name):
    if not (t.is_cuda and t.dtype == torch.int8):
        raise ValueError(f"{name}: an int8 CUDA tensor")


def _scale(v, name):
    v = float(v)
    if not (v > 0.0 and v < float("inf")):
        raise ValueError(f"{name}: a positive finite scale, got {v}")
    return v


def quantize_weight_taps(weight, bias=None, groups_in=None, groups_out=None, multiple=CHANNEL_MULTIPLE):
    """Per-output-channel min-max quantisation of a convolution weight [Cout, Cin, k, k] for conv_slice_q_taps, after
    the padding of `pad_channels`: -> (w_q_taps int8 [Pout, k, k, Pin], w_scales fp32 [Pout], bias fp32 [Pout]).
    scale[co] = amax_co / 127 in fp32 (1 for a row of zeros: the pad rows), q = clamp(rne(w / scale), -127, 127) with
    the quotient in fp32; pad rows and columns are exact zeros and the pad bias is zero, so a pad channel leaves a layer
    as q = 0."""
    wp, bp = pad_channels(weight.detach().float(), None if bias is None else bias.detach().float(), groups_in, groups_out,
                          multiple)
    amax = wp.abs().amax(dim=(1, 2, 3))
    scales = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    q = torch.clamp(torch.round(wp / scales[:, None, None, None]), -127, 127).to(torch.int8)
    if bp is None:
        bp = wp.new_zeros((wp.shape[0],))
    return q.permute(0, 2, 3, 1).contiguous(), scales.contiguous(), bp.contiguous()


def conv_slice_q_taps(x_q, scale_x, w_q_taps, w_scales, bias, act, residual_q=None, scale_res=1.0, stride=1, out=None,
                      scale_out=None, out_dtype=torch.int8, res_first=False, dilation=1, image_bias=None):
    """bevops_conv_slice_s8(_ex, _ex2): the convolution of an int8 channel slice x_q [B, Cin, H, W] (real = q scale_x) with int8
    taps-major weights w_q_taps [Cout, k, k, Cin] (real = q w_scales[co]; w_scales fp32 [Cout]), bias fp32 [Cout] or
    None, act in "none", "relu", "silu", the int8 identity residual_q (real = q scale_res) added BEHIND the
    activation -- or, with res_first=True (act "none" / "relu" and an identity, else BevopsError NOT_SUPPORTED), IN FRONT of
    it: act(conv + bias + identity), mmdet's BasicBlock.  out_dtype torch.int8: requantised with scale_out, q = clamp(rne(v / scale_out), -127, 127);
    torch.float16: one rounding (scale_out unused).  Cin % 32 == 0, Cout % 16 == 0 (int8 out) or % 8 (fp16 out), k in
    {1, 3}, stride in {1, 2}, else BevopsError NOT_SUPPORTED.  include/bevops.h states the operation order.
    dilation > 1 (bevops_conv_slice_s8_ex2): k == 3 and stride == 1, pad = dilation, else BevopsError NOT_SUPPORTED.
    image_bias [B, P] fp16 (P >= Cout, P % 8 == 0, rows contiguous): a bias per IMAGE in place of `bias` -- output pixel
    (b, y, x) takes image_bias[b, co].  With the defaults the call is bevops_conv_slice_s8_ex's."""
    _check_s8(x_q, "x_q")
    if w_q_taps.dim() != 4 or w_q_taps.shape[1] != w_q_taps.shape[2] or not w_q_taps.is_contiguous() or \
            w_q_taps.dtype != torch.int8 or w_q_taps.device != x_q.device:
        raise ValueError("conv_slice_q: w_q_taps [Cout, k, k, Cin] contiguous int8 on the input's device")
    B, Cin, H, W = x_q.shape
    Cout, k = w_q_taps.shape[0], w_q_taps.shape[1]
    if w_q_taps.shape[3] != Cin:
        raise ValueError(f"conv_slice_q: the weight has {w_q_taps.shape[3]} input channels, x_q has {Cin}")
    if act not in ACTS:
        raise ValueError(f"conv_slice_q: act in {sorted(k for k in ACTS if k)}")
    if out_dtype not in (torch.int8, torch.float16):
        raise ValueError("conv_slice_q: out_dtype torch.int8 or torch.float16")
    if out is not None and out.dtype != out_dtype:
        raise ValueError(f"conv_slice_q: out is {out.dtype}, out_dtype {out_dtype}")
    out8 = out_dtype == torch.int8
    if k not in (1, 3) or stride not in (1, 2) or Cin % 32 or Cout % (16 if out8 else 8):
        raise _lib.BevopsError("bevops_conv_slice_s8: ksize in {1, 3}, stride in {1, 2}, Cin % 32 == 0, Cout % 16 == 0 "
                               "(int8 out) or % 8 (fp16 out)", _lib.NOT_SUPPORTED)
    sx = _scale(scale_x, "scale_x")
    so = _scale(scale_out, "scale_out") if out8 else 1.0
    for t, name in ((w_scales, "w_scales"), (bias, "bias")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != Cout or
                              t.device != x_q.device):
            raise ValueError(f"conv_slice_q: {name} contiguous fp32 [Cout] on the input's device")
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    xp = slice_pitch(x_q, "x_q")
    if out is None:
        out = nhwc_empty(B, Cout, Ho, Wo, x_q.device, out_dtype)
    elif tuple(out.shape) != (B, Cout, Ho, Wo) or out.device != x_q.device:
        raise ValueError(f"conv_slice_q: out must be {(B, Cout, Ho, Wo)} on {x_q.device}, got {tuple(out.shape)}")
    op = slice_pitch(out, "out")
    rp, sr = 0, 1.0
    if residual_q is not None:
        _check_s8(residual_q, "residual_q")
        if tuple(residual_q.shape) != tuple(out.shape):
            raise ValueError("conv_slice_q: the identity has the output's shape")
        rp, sr = slice_pitch(residual_q, "residual_q"), _scale(scale_res, "scale_res")
    if res_first and (residual_q is None or act == "silu"):
        raise _lib.BevopsError("bevops_conv_slice_s8_ex: res_first needs an identity and act none / relu", _lib.NOT_SUPPORTED)
    dilation = int(dilation)
    if dilation < 1:
        raise ValueError("conv_slice_q: dilation >= 1")
    if dilation > 1 and (k != 3 or stride != 1):
        raise _lib.BevopsError("bevops_conv_slice_s8_ex2: dilation > 1 needs ksize 3 and stride 1", _lib.NOT_SUPPORTED)
    bp = 0
    if image_bias is not None:
        if bias is not None:
            raise ValueError("conv_slice_q: image_bias replaces bias, pass one of them")
        _check_f16(image_bias, "image_bias")
        if image_bias.dim() != 2 or image_bias.shape[0] != B or image_bias.shape[1] < Cout or \
                (image_bias.shape[1] > 1 and image_bias.stride(1) != 1) or image_bias.device != x_q.device:
            raise ValueError(f"conv_slice_q: image_bias [B, >= Cout] with contiguous rows, got {tuple(image_bias.shape)}")
        bp = image_bias.stride(0) if B > 1 else padded_width(image_bias.shape[1], 8)
        if bp < Cout or bp % 8 or image_bias.data_ptr() % 16:
            raise ValueError(f"conv_slice_q: image_bias rows start on 16-byte boundaries, pitch a multiple of 8 (pitch {bp})")
    if B == 0:
        return out
    if dilation > 1 or image_bias is not None:
        _call("bevops_conv_slice_s8_ex2", x_q.device, x_q.data_ptr(), xp, sx, w_q_taps.data_ptr(), _ptr(w_scales), 1.0,
              _ptr(bias), _ptr(residual_q), rp, sr, _lib.I8 if out8 else _lib.F16, out.data_ptr(), op, so, B, H, W, Cin,
              Cout, k, int(stride), ACTS[act], int(bool(res_first)), dilation, _ptr(image_bias), bp)
        return out
    _call("bevops_conv_slice_s8_ex", x_q.device, x_q.data_ptr(), xp, sx, w_q_taps.data_ptr(), _ptr(w_scales), 1.0,
          _ptr(bias), _ptr(residual_q), rp, sr, _lib.I8 if out8 else _lib.F16, out.data_ptr(), op, so, B, H, W, Cin, Cout, k,
          int(stride), ACTS[act], int(bool(res_first)))
    return out


def focus_nhwc_q(image, scale, out=None):
    """`focus_nhwc` leaving as int8 (bevops_focus_nhwc_q): image [B, 3, H, W] contiguous fp16 -> an int8 channel slice
    [B, 32, H/2, W/2], q = clamp(rne(x / scale), -127, 127) (the product x * (1 / scale) in fp32), channels 12 .. 31
    zero."""
    _check_f16(image, "image")
    if image.dim() != 4 or image.shape[1] != 3 or not image.is_contiguous():
        raise ValueError("focus_nhwc_q: a contiguous [B, 3, H, W] image")
    B, _, H, W = image.shape
    if H % 2 or W % 2:
        raise _lib.BevopsError("bevops_focus_nhwc_q: H and W even", _lib.NOT_SUPPORTED)
    s = _scale(scale, "scale")
    shape = (B, FOCUS_CHANNELS, H // 2, W // 2)
    if out is None:
        out = nhwc_empty(*shape, image.device, torch.int8)
    elif tuple(out.shape) != shape or out.dtype != torch.int8 or out.device != image.device:
        raise ValueError(f"focus_nhwc_q: out must be {shape} int8 on {image.device}, got {tuple(out.shape)}")
    op = slice_pitch(out, "out")
    if B:
        _call("bevops_focus_nhwc_q", image.device, image.data_ptr(), s, out.data_ptr(), op, B, H, W)
    return out


def _spp_maxpool_s8(x, out, kernel_sizes):
    _check_s8(x, "x")
    B, C, H, W = x.shape
    ks = tuple(int(k) for k in kernel_sizes)
    if len(ks) != 3:
        raise ValueError("spp_maxpool_nhwc: three kernel sizes")
    if C % 16 or any(k % 2 == 0 or k > 13 or k < 1 for k in ks):
        raise _lib.BevopsError("bevops_spp_maxpool_nhwc_s8: C % 16 == 0, odd kernel sizes <= 13", _lib.NOT_SUPPORTED)
    xp = slice_pitch(x, "x")
    out = _dest(out, (B, 3 * C, H, W), x, "spp_maxpool_nhwc")
    op = slice_pitch(out, "out")
    if B:
        _call("bevops_spp_maxpool_nhwc_s8", x.device, x.data_ptr(), xp, out.data_ptr(), op, B, H, W, C, *ks)
    return out
