"""3-D convolution on CHANNEL SLICES of channels-last fp16 volumes (bevops_conv3d_slice_f16, csrc/conv3d_slice.hip,
design/conv3d.md): the layers of BEVDet-Occ's 3-D BEV encoder (bevformer_tensorrt_amd/bevdet_occ3d.py).  Not a reference
plugin (the reference tree has no 3-D convolution).

    out = act(conv3d(x, weight, stride, pad k // 2) + bias + residual)      the identity IN FRONT OF the activation

A channel slice is a [B, C, Z, Y, X] view `buf[:, c0:c0 + C]` of a `torch.channels_last_3d` tensor `buf` [B, Ct, Z, Y, X]:
strides (Z Y X Ct, 1, Y X Ct, X Ct, Ct).  Ct is the slice's PITCH; a slice starts on a 16-byte boundary (c0 % 8 == 0) and
its pitch is a multiple of 8.  With `out=` a layer writes its slice of a wider buffer (LSSFPN3D's concatenation)."""
import torch
import torch.nn.functional as F

from ..utils import lib as _lib
from .linear import _call, _ptr
from .multi_scale_deformable_attn import _TensorCache

ACTS3D = {None: 0, "none": 0, "relu": 1}
_TAPS = _TensorCache()   # weight [Cout, Cin, k, k, k] -> its taps-major copy


def ndhwc_empty(B, C, Z, Y, X, device, dtype=torch.float16):
    """An uninitialised channels-last volume [B, C, Z, Y, X] with explicit strides (Z Y X C, 1, Y X C, X C, C) for every
    size, unit axes included."""
    return torch.empty((B, Z, Y, X, C), device=device, dtype=dtype).permute(0, 4, 1, 2, 3)


def volume_pitch(t):
    """The pitch (elements between two voxels) of a channel slice of a channels-last volume, or None when `t` is not one
    (layout, 16-byte alignment of the slice, pitch a multiple of 8)."""
    if t.dim() != 5:
        return None
    B, C, Z, Y, X = t.shape
    want, pitch = 1, None
    for n, s in ((X, t.stride(4)), (Y, t.stride(3)), (Z, t.stride(2)), (B, t.stride(0))):
        if n > 1:
            pitch = s // want if pitch is None else pitch
            if s != want * pitch:
                return None
        want *= n
    if pitch is None:
        pitch = (C + 7) // 8 * 8
    if pitch < C or (C > 1 and t.stride(1) != 1) or pitch % 8 or t.data_ptr() % 16:
        return None
    return pitch


def conv3d_taps_weight(weight, build=True):
    """The taps-major operand [Cout, kz, ky, kx, Cin] of bevops_conv3d_slice_f16 for `weight` [Cout, Cin, k, k, k]:
    taps[co, kz, ky, kx, ci] = weight[co, ci, kz, ky, kx].  Cached per weight tensor, rebuilt when the weight changes;
    build=False: None when missing or stale.  Never built inside a stream capture (RuntimeError)."""
    hit = _TAPS.get(weight)
    if hit is not None or not build:
        return hit
    if weight.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("conv3d_ndhwc: the taps-major weight is missing or stale and the stream is capturing; call "
                           "conv3d_taps_weight(weight) (or the layer once, eagerly) before the capture")
    return _TAPS.put(weight, weight.detach().permute(0, 2, 3, 4, 1).contiguous())


def conv3d_plain(x, weight, bias=None, act="relu", residual=None, stride=1):
    """The statement in torch, in x's dtype on x's device: act(F.conv3d(x, weight, stride, pad k // 2) + bias + residual)."""
    v = F.conv3d(x, weight.to(x.dtype), None, stride, weight.shape[2] // 2)
    if bias is not None:
        v = v + bias.to(x.dtype).view(1, -1, 1, 1, 1)
    if residual is not None:
        v = v + residual
    return F.relu(v) if ACTS3D[act] else v


def _fast(*tensors):
    return all(t is None or (t.is_cuda and t.dtype == torch.float16 and volume_pitch(t) is not None) for t in tensors)


def conv3d_taps(x, weight_taps, bias=None, act="relu", residual=None, stride=1, out=None):
    """`conv3d_ndhwc` on a weight that already is taps-major: weight_taps [Cout, kz, ky, kx, Cin] contiguous, k in {1, 3},
    Cin == x.shape[1]."""
    if weight_taps.dim() != 5 or len(set(weight_taps.shape[1:4])) != 1 or weight_taps.shape[4] != x.shape[1]:
        raise ValueError("conv3d: weight_taps [Cout, k, k, k, Cin] with x's channels")
    if act not in ACTS3D:
        raise ValueError("conv3d: act in 'none', 'relu'")
    if x.dim() != 5:
        raise ValueError("conv3d: x [B, C, Z, Y, X]")
    B, Cin, Z, Y, X = x.shape
    Cout, k = weight_taps.shape[0], weight_taps.shape[1]
    pad = k // 2
    shape = (B, Cout) + tuple((n + 2 * pad - k) // stride + 1 for n in (Z, Y, X))
    if residual is not None and tuple(residual.shape) != shape:
        raise ValueError("conv3d: the identity has the output's shape")
    if out is not None and (tuple(out.shape) != shape or out.dtype != x.dtype or out.device != x.device):
        raise ValueError(f"conv3d: out must be {shape} {x.dtype} on {x.device}, got {tuple(out.shape)}")
    if bias is not None and bias.numel() != Cout:
        raise ValueError("conv3d: one bias per output channel")
    if not _fast(x, residual, out):
        y = conv3d_plain(x, weight_taps.permute(0, 4, 1, 2, 3), bias, act, residual, stride)
        return y if out is None else out.copy_(y)
    if weight_taps.dtype != torch.float16 or weight_taps.device != x.device or not weight_taps.is_contiguous():
        raise ValueError("conv3d: weight_taps contiguous fp16 on the input's device")
    if k not in (1, 3) or stride not in (1, 2) or Cin % 32 or Cout % 8:
        raise _lib.BevopsError("bevops_conv3d_slice_f16: ksize in {1, 3}, stride in {1, 2}, Cin % 32 == 0, Cout % 8 == 0",
                               _lib.NOT_SUPPORTED)
    if out is None:
        out = ndhwc_empty(*shape, x.device)
    if bias is not None and (bias.dtype != torch.float16 or not bias.is_contiguous() or bias.data_ptr() % 16):
        bias = bias.detach().to(torch.float16).clone()
    if B:
        _call("bevops_conv3d_slice_f16", x.device, x.data_ptr(), volume_pitch(x), weight_taps.data_ptr(), _ptr(bias),
              _ptr(residual), volume_pitch(residual) if residual is not None else 0, out.data_ptr(), volume_pitch(out),
              B, Z, Y, X, Cin, Cout, k, int(stride), ACTS3D[act])
    return out


def conv3d_ndhwc(x, weight, bias=None, act="relu", residual=None, stride=1, out=None):
    """out = act(conv3d(x, weight, stride, pad k // 2) + bias + residual), the identity IN FRONT OF the activation.
    x [B, Cin, Z, Y, X], residual and out [B, Cout, Zo, Yo, Xo]: fp16 CUDA channel slices of channels-last volumes;
    weight [Cout, Cin, k, k, k] with k in {1, 3}; stride in {1, 2} on all three axes; act in "none", "relu".  Cin % 32 == 0
    and Cout % 8 == 0 (else BevopsError NOT_SUPPORTED).  Without `out=` a new channels-last volume is returned.  CPU
    tensors, fp32 tensors and tensors that are no channel slices of channels-last volumes take `conv3d_plain`."""
    if weight.dim() != 5 or len(set(weight.shape[2:])) != 1:
        raise ValueError("conv3d_ndhwc: weight [Cout, Cin, k, k, k]")
    if not _fast(x, residual, out):
        y = conv3d_plain(x, weight, bias, act, residual, stride)
        return y if out is None else out.copy_(y)
    return conv3d_taps(x, conv3d_taps_weight(weight), bias, act, residual, stride, out)
