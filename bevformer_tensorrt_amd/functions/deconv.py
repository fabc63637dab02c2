"""ConvTranspose2d(C, C', 4, stride 2, padding 1) + bias + ReLU of the channels-last fp16 path (the up-sampling layers of
mmdet's CTResNetNeck) as four implicit GEMMs on the matrix cores, one per output parity (bevops_deconv4x4s2_f16,
csrc/deconv.hip): no column buffer, no zero-stuffed input, bias and ReLU in the epilogue, one rounding.  Not a reference
plugin (TensorRT owns the layer there)."""
import torch

from ..utils import lib as _lib
from .linear import _call, _ptr
from .multi_scale_deformable_attn import _TensorCache

_PACKED = _TensorCache()   # weight tensor -> parity-major packed copy (weakly keyed and stamped, as conv.pack_taps')


def deconv4x4s2_tap(py, px, dy, dx):
    """Output pixel (2 y + py, 2 x + px) sums four taps (dy, dx) in {0, 1}^2: input pixel (y - 1 + py + dy,
    x - 1 + px + dx) times weight[:, :, ky, kx] -> ((row offset, column offset), (ky, kx))."""
    return (py + dy - 1, px + dx - 1), (3 - py - 2 * dy, 3 - px - 2 * dx)


def pack_deconv4x4s2(weight):
    """[Cin, Cout, 4, 4] (ConvTranspose2d's layout) -> [4 parities, Cout, 2, 2, Cin] contiguous: parity 2 py + px is a
    row-major [Cout, K = 4 Cin] GEMM operand with k ordered [dy][dx][Cin].  Any device / dtype; not cached."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (4, 4):
        raise ValueError("pack_deconv4x4s2: a [Cin, Cout, 4, 4] weight")
    cin, cout = weight.shape[:2]
    w = weight.detach()
    packed = w.new_empty((4, cout, 2, 2, cin))
    for py in range(2):
        for px in range(2):
            for dy in range(2):
                for dx in range(2):
                    _, (ky, kx) = deconv4x4s2_tap(py, px, dy, dx)
                    packed[2 * py + px, :, dy, dx, :] = w[:, :, ky, kx].t()
    return packed


def deconv_packed_weight(weight, build=True):
    """`pack_deconv4x4s2(weight)` cached per weight tensor the way functions.conv.pack_taps caches the taps-major
    copies; rebuilt when the weight changes.  build=False: None when the cached copy is missing or stale.  Packing
    allocates and copies: never inside a stream capture (RuntimeError)."""
    hit = _PACKED.get(weight)
    if hit is None and build:
        if weight.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("conv_transpose2d_nhwc: the packed weight is missing or stale and the stream is capturing; "
                               "call deconv_packed_weight(weight) (or the layer once, eagerly) before the capture")
        hit = _PACKED.put(weight, pack_deconv4x4s2(weight))
    return hit


def conv_transpose2d_nhwc(x, weight, bias=None, relu=False):
    """x [B, Cin, H, W] channels-last fp16, weight [Cin, Cout, 4, 4] -> act(conv_transpose2d(x, weight, stride 2,
    padding 1) + bias) [B, Cout, 2H, 2W] channels-last.  Cin % 32 == 0, Cout % 8 == 0 (else BevopsError NOT_SUPPORTED)."""
    assert x.is_cuda and x.dtype == torch.float16 and x.dim() == 4
    assert x.is_contiguous(memory_format=torch.channels_last)
    B, Cin, H, W = x.shape
    if weight.dim() != 4 or weight.shape[0] != Cin or tuple(weight.shape[2:]) != (4, 4):
        raise ValueError("conv_transpose2d_nhwc: weight [Cin, Cout, 4, 4] matching the input channels")
    if weight.dtype != torch.float16 or weight.device != x.device:
        raise ValueError("conv_transpose2d_nhwc: an fp16 weight on the input's device")
    Cout = weight.shape[1]
    if Cin % 32 or Cout % 8:       # (before the pack, which does not care)
        raise _lib.BevopsError("bevops_deconv4x4s2_f16: Cin % 32 == 0 and Cout % 8 == 0", _lib.NOT_SUPPORTED)
    wp = deconv_packed_weight(weight)
    out = torch.empty((B, Cout, 2 * H, 2 * W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    if bias is not None:
        bias = bias.to(torch.float16).contiguous()
    if B == 0:
        return out
    _call("bevops_deconv4x4s2_f16", x.device, _lib.F16, x.data_ptr(), wp.data_ptr(), _ptr(bias), out.data_ptr(), B, H, W,
          Cin, Cout, 4, 2, 1, int(bool(relu)))
    return out


# ---- the INT8 flavour (the INT8 build of CenterNet, quantization.build_int8_centernet)

def quantize_deconv_weight(weight, bias=None):
    """Per-output-channel min-max quantisation of a transposed convolution's weight [Cin, Cout, 4, 4] (the per-channel
    axis is dimension 1): -> (weight_q int8 [Cin, Cout, 4, 4], w_scales fp32 [Cout], bias fp32 [Cout]).  scale[co] =
    amax_co / 127 in fp32 (1 for a channel of zeros), q = clamp(rne(w / scale), -127, 127), the quotient in fp32."""
    w = weight.detach().float()
    amax = w.abs().amax(dim=(0, 2, 3))
    scales = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    q = torch.clamp(torch.round(w / scales[None, :, None, None]), -127, 127).to(torch.int8)
    b = w.new_zeros((w.shape[1],)) if bias is None else bias.detach().float()
    return q.contiguous(), scales.contiguous(), b.contiguous()


def conv_transpose2d_q_nhwc(x_q, scale_x, weight_q, w_scales, bias, relu, scale_out=None, out_dtype=torch.int8):
    """bevops_deconv4x4s2_s8: x_q [B, Cin, H, W] channels-last int8 (real = q scale_x), weight_q int8 [Cin, Cout, 4, 4]
    (real = q w_scales[co]; w_scales fp32 [Cout] or None), bias fp32 [Cout] or None -> act(conv_transpose2d(x, w, stride 2,
    padding 1) + bias) [B, Cout, 2H, 2W] channels-last.  out_dtype torch.int8: requantised with scale_out,
    q = clamp(rne(v / scale_out), -127, 127); torch.float16: one rounding (scale_out unused).  Cin % 64 == 0, Cout % 16
    == 0 (int8 out) or % 8 (fp16 out), else BevopsError NOT_SUPPORTED.  The parity-major packed int8 weight is cached per
    weight tensor like the fp16 one (deconv_packed_weight): never built inside a stream capture.  include/bevops.h
    states the operation order."""
    if not (x_q.is_cuda and x_q.dtype == torch.int8 and x_q.dim() == 4):
        raise ValueError("conv_transpose2d_q_nhwc: x_q an int8 CUDA tensor [B, Cin, H, W]")
    if not x_q.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("conv_transpose2d_q_nhwc: x_q channels-last")
    B, Cin, H, W = x_q.shape
    if weight_q.dim() != 4 or weight_q.shape[0] != Cin or tuple(weight_q.shape[2:]) != (4, 4):
        raise ValueError("conv_transpose2d_q_nhwc: weight_q [Cin, Cout, 4, 4] matching the input channels")
    if weight_q.dtype != torch.int8 or weight_q.device != x_q.device:
        raise ValueError("conv_transpose2d_q_nhwc: an int8 weight on the input's device")
    if out_dtype not in (torch.int8, torch.float16):
        raise ValueError("conv_transpose2d_q_nhwc: out_dtype torch.int8 or torch.float16")
    Cout = weight_q.shape[1]
    out8 = out_dtype == torch.int8
    if Cin % 64 or Cout % (16 if out8 else 8):       # (before the pack, which does not care)
        raise _lib.BevopsError("bevops_deconv4x4s2_s8: Cin % 64 == 0, Cout % 16 == 0 (int8 out) or % 8 (fp16 out)",
                               _lib.NOT_SUPPORTED)

    def scale(v, name):
        v = float(v)
        if not (v > 0.0 and v < float("inf")):
            raise ValueError(f"conv_transpose2d_q_nhwc: {name} a positive finite scale, got {v}")
        return v

    sx = scale(scale_x, "scale_x")
    so = scale(scale_out, "scale_out") if out8 else 1.0
    for t, name in ((w_scales, "w_scales"), (bias, "bias")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != Cout or
                              t.device != x_q.device):
            raise ValueError(f"conv_transpose2d_q_nhwc: {name} contiguous fp32 [Cout] on the input's device")
    wp = deconv_packed_weight(weight_q)
    out = torch.empty((B, Cout, 2 * H, 2 * W), dtype=out_dtype, device=x_q.device, memory_format=torch.channels_last)
    if B == 0:
        return out
    _call("bevops_deconv4x4s2_s8", x_q.device, x_q.data_ptr(), sx, wp.data_ptr(), _ptr(w_scales), 1.0, _ptr(bias),
          _lib.I8 if out8 else _lib.F16, out.data_ptr(), so, B, H, W, Cin, Cout, int(bool(relu)))
    return out
