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
