"""The front of a plain LSS view transformer -- depth_net (a 1 x 1 convolution to D depth logits + C context features),
the softmax over the depth bins and the two slice / permute copies -- as ONE launch of bevops_lss_depth_head_f16
(csrc/depth_head.hip, design/depth_head.md): the logits stay fp32 accumulators in registers, the launch writes both
operands of bev_pool_v2.  Serves C + D <= 256 columns.  Not a reference plugin (TensorRT owns these layers there), so
not in TRT_FUNCTIONS.

Argument checks as in functions.bev_half: a wrong type or dtype raises TypeError, a shape or layout outside the entry's
domain ValueError, a tensor that is not on the GPU TypeError (checked last)."""
from collections import namedtuple

import torch

from .bev_half import _fp16, _on_gpu
from .linear import _call
from .multi_scale_deformable_attn import _TensorCache

DepthHeadPacked = namedtuple("DepthHeadPacked", "w bias Cin C D nt")
_PACKED = _TensorCache()   # weight -> (stamp of the bias, D, C; DepthHeadPacked)


def depth_head_supported(Cin, C, D):
    """The domain of bevops_lss_depth_head_f16 (include/bevops.h)."""
    return Cin % 32 == 0 and 32 <= Cin <= 512 and C % 8 == 0 and 8 <= C <= 128 and D >= 1 and C + D <= 256


def pack_depth_head_tensors(weight, bias, D, C):
    """weight [D + C, Cin(, 1, 1)] and bias [D + C] or None (depth rows first, as nn.Conv2d(Cin, D + C, 1) holds them; any
    device / float dtype) -> DepthHeadPacked: w fp16 [nt, Cin / 16, 64, 8] in fragment order and bias fp32 [32 nt], columns
    [features | depth bins | zeros] (include/bevops.h).  Not cached."""
    D, C = int(D), int(C)
    w2 = weight.detach().reshape(weight.shape[0], -1)
    Cin = w2.shape[1]
    if w2.shape[0] != D + C or (bias is not None and bias.numel() != D + C):
        raise ValueError(f"pack_depth_head: weight [D + C, Cin] and bias [D + C] for D = {D}, C = {C}, got "
                         f"{tuple(weight.shape)}")
    if not depth_head_supported(Cin, C, D):
        raise ValueError(f"pack_depth_head: Cin = {Cin}, C = {C}, D = {D} outside Cin % 32 == 0 in [32, 512], C % 8 == 0 in "
                         "[8, 128], D >= 1, C + D <= 256")
    nt = (C + D + 31) // 32
    cols = w2.new_zeros((32 * nt, Cin), dtype=torch.float16)
    cols[:C] = w2[D:]
    cols[C:C + D] = w2[:D]
    b = w2.new_zeros((32 * nt,), dtype=torch.float32)
    if bias is not None:
        b[:C] = bias.detach()[D:]
        b[C:C + D] = bias.detach()[:D]
    # lane l = 32 hb + r of (tile t, k-step s): column 32 t + r, k = 16 s + 8 hb .. + 7
    w = cols.view(nt, 32, Cin // 16, 2, 8).permute(0, 2, 3, 1, 4).reshape(nt, Cin // 16, 64, 8).contiguous()
    return DepthHeadPacked(w, b, Cin, C, D, nt)


def pack_depth_head(weight, bias, D, C, build=True):
    """`pack_depth_head_tensors` cached per weight tensor (stamped with the bias, D and C, as pack_occ_head's cache);
    rebuilt when weight or bias changes.  build=False: None when missing or stale.  Packing allocates and copies: never
    inside a stream capture (RuntimeError)."""
    stamp = (_TensorCache._stamp(weight), None if bias is None else _TensorCache._stamp(bias), int(D), int(C))
    hit = _PACKED.get(weight)
    if hit is not None and hit[0] == stamp:
        return hit[1]
    if not build:
        return None
    if weight.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("lss_depth_head: the packed depth_net is missing or stale and the stream is capturing; call "
                           "pack_depth_head(...) (or the layer once, eagerly) before the capture")
    return _PACKED.put(weight, (stamp, pack_depth_head_tensors(weight, bias, D, C)))[1]


def lss_depth_head(x, packed, n, spatial=None, out=None):
    """x [n * hw, Cin] fp16 pixel rows with a unit channel stride (a channels-last activation viewed as rows; the row
    pitch may exceed Cin), packed = pack_depth_head(...)  ->  (depth [n, D, hw], feat [n, hw, C]), what `lss_depth_split`
    returns behind depth_net; spatial=(H, W) with H * W == hw: [n, D, H, W] and [n, H, W, C].  out=(depth, feat): dense
    fp16 tensors of those shapes to fill."""
    _fp16(x, "lss_depth_head: x")
    if not isinstance(packed, DepthHeadPacked):
        raise TypeError(f"lss_depth_head: packed must come from pack_depth_head, got {type(packed).__name__}")
    if out is not None:
        for t, what in zip(out, ("depth", "feat")):
            _fp16(t, f"lss_depth_head: out {what}")
    n = int(n)
    if x.dim() != 2 or x.shape[1] != packed.Cin or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError(f"lss_depth_head: x must be [rows, {packed.Cin}] with a unit channel stride, got "
                         f"{tuple(x.shape)} / {x.stride()}")
    rows = x.shape[0]
    pitch = x.stride(0) if rows > 1 else packed.Cin
    if pitch < packed.Cin or pitch % 8:
        raise ValueError(f"lss_depth_head: the row pitch {pitch} must be a multiple of 8 and at least Cin")
    if n < 0 or (n == 0 and rows != 0) or (n > 0 and rows % n != 0):
        raise ValueError(f"lss_depth_head: {rows} rows do not split into n = {n} images")
    hw = rows // n if n > 0 else 0
    if spatial is not None and int(spatial[0]) * int(spatial[1]) != hw:
        raise ValueError(f"lss_depth_head: spatial = {tuple(spatial)} does not match {hw} pixels per image")
    D, C = packed.D, packed.C
    dshape, fshape = ((n, D, hw), (n, hw, C)) if spatial is None else \
        ((n, D, int(spatial[0]), int(spatial[1])), (n, int(spatial[0]), int(spatial[1]), C))
    if out is not None and not (tuple(out[0].shape) == dshape and tuple(out[1].shape) == fshape
                                and out[0].is_contiguous() and out[1].is_contiguous()):
        raise ValueError(f"lss_depth_head: out must be dense tensors {dshape} and {fshape}")
    _on_gpu(x, "lss_depth_head: x")
    if packed.w.device != x.device or (out is not None and (out[0].device != x.device or out[1].device != x.device)):
        raise TypeError("lss_depth_head: x, the packed weights and out are on different devices")
    depth, feat = out if out is not None else (torch.empty(dshape, dtype=x.dtype, device=x.device),
                                               torch.empty(fshape, dtype=x.dtype, device=x.device))
    if rows:
        _call("bevops_lss_depth_head_f16", x.device, x.data_ptr(), pitch, packed.w.data_ptr(), packed.bias.data_ptr(),
              depth.data_ptr(), feat.data_ptr(), n, hw, packed.Cin, C, D)
    return depth, feat


def lss_depth_head_plain(x, weight, bias, D, C, n, spatial=None):
    """The statement in torch, in x's dtype, on x's device: x [n * hw, Cin] rows, weight [D + C, Cin(, 1, 1)] with the
    depth rows first -> (depth [n, D, hw] = softmax over each pixel's D logits, feat [n, hw, C]); `spatial` as above."""
    w = weight.detach().reshape(weight.shape[0], -1).to(x.dtype)
    v = x @ w.t()
    if bias is not None:
        v = v + bias.detach().to(x.dtype)
    hw = x.shape[0] // n if n else 0
    depth = v[:, :D].softmax(dim=1).reshape(n, hw, D).permute(0, 2, 1).contiguous()
    feat = v[:, D:D + C].reshape(n, hw, C).contiguous()
    if spatial is not None:
        depth, feat = depth.view(n, D, *spatial), feat.view(n, *spatial, C)
    return depth, feat
